# Fake-tensor tests: fake CUDA construction on GPU-less CI, guard
# teardown, ops/views/autograd on fake tensors, meta_like metadata, the
# documented output-device heuristic (explicit device arg -> common
# tensor device -> CPU, with the 0-dim CPU scalar exemption), and repr.
# tests/test_reference_suite.py checks that the `torchdistx` alias exports
# these very objects.

import pytest
import torch

from torchdistx_amd.fake import fake_mode, is_fake, meta_like

requires_no_gpu = pytest.mark.skipif(
    torch.cuda.is_available(),
    reason="exercises the fake-CUDA guard, which is inert with a real GPU",
)


@requires_no_gpu
def test_fake_cuda_guard_lifecycle() -> None:
    # On a GPU-less box, "cuda" factories fail unless fake_cuda installs
    # the no-op device guard...
    with pytest.raises((AssertionError, RuntimeError)):
        with fake_mode():
            torch.empty([2, 2], device="cuda")

    # ...with it, construction succeeds and reports a concrete cuda device.
    with fake_mode(fake_cuda=True):
        t = torch.empty([2, 2], device="cuda")
    assert is_fake(t)
    assert t.device.type == "cuda"
    assert t.device.index == 0

    # Leaving the mode tears the guard down: real cuda work fails again.
    with pytest.raises((AssertionError, RuntimeError)):
        torch.empty([2, 2], device="cuda")


def test_fake_cpu_tensor_has_no_storage() -> None:
    with fake_mode():
        a = torch.ones([4, 4])

    assert is_fake(a)
    assert a.device.type == "cpu"
    assert a.shape == (4, 4)
    with pytest.raises(RuntimeError):
        a.untyped_storage()


def test_ops_on_fake_tensors_stay_fake() -> None:
    with fake_mode():
        a = torch.ones([4, 4])
        b = a + a
        c = b.view(16)
        d = c[:8]
    assert is_fake(b) and is_fake(c) and is_fake(d)
    assert d.shape == (8,)


@requires_no_gpu
def test_fake_cuda_ops_report_cuda_device() -> None:
    with fake_mode(fake_cuda=True):
        a = torch.zeros([8], device="cuda")
        b = a * 2 + 1
    assert b.device.type == "cuda"
    assert is_fake(b)


def test_real_tensors_unaffected_inside_fake_mode() -> None:
    r = torch.ones([3])
    with fake_mode():
        s = r.sum()
    # `r` is real, so the computation ran for real.
    assert not is_fake(r)
    assert s.item() == pytest.approx(3.0)


def test_meta_like_copies_metadata_without_fake_key() -> None:
    with fake_mode():
        src = torch.ones([6, 2], dtype=torch.float16).t()

    m = meta_like(src)

    assert m.is_meta
    assert not is_fake(m)
    assert (m.dtype, tuple(m.shape), tuple(m.stride())) == (
        src.dtype,
        tuple(src.shape),
        tuple(src.stride()),
    )


def test_meta_like_rejects_real_tensors() -> None:
    with pytest.raises(ValueError):
        meta_like(torch.zeros([5]))


def test_fake_repr_mentions_fake() -> None:
    with fake_mode():
        a = torch.ones([2, 3], dtype=torch.float64)
    r = repr(a)
    assert "fake=True" in r
    assert "size=(2, 3)" in r
    # Real tensors keep the stock repr.
    assert "fake" not in repr(torch.ones([1]))


def test_fake_mode_nesting() -> None:
    with fake_mode():
        with fake_mode():
            a = torch.ones([2])
        b = torch.ones([2])
    assert is_fake(a) and is_fake(b)
    assert not is_fake(torch.ones([2]))


def test_backward_through_fake_tensors() -> None:
    # Autograd runs above the Fake key, so backward works end-to-end on
    # fake tensors and produces fake gradients.
    with fake_mode():
        x = torch.randn(4, 4, requires_grad=True)
        y = (x * 2).sum()
        y.backward()
    assert x.grad is not None
    assert is_fake(x.grad)
    assert x.grad.shape == (4, 4)


# ---------------------------------------------------------------------------
# Output-device heuristic (reference docs
# fake_tensor_and_deferred_init.rst:120-137): explicit device argument of a
# device-consuming op > common tensor-arg device > CPU; tensor args on two
# devices are an error, except 0-dim CPU scalars.
# ---------------------------------------------------------------------------


@requires_no_gpu
def test_mixed_device_tensor_args_raise() -> None:
    with fake_mode(fake_cuda=True):
        a = torch.ones([4], device="cuda")
        cpu_vec = torch.ones([4])  # fake CPU, 1-dim: not a scalar
        with pytest.raises(RuntimeError, match="common device"):
            a + cpu_vec


@requires_no_gpu
def test_cpu_scalar_exemption() -> None:
    scale = torch.tensor(2.0)  # real 0-dim CPU scalar
    with fake_mode(fake_cuda=True):
        a = torch.ones([4], device="cuda")
        b = a * scale
    assert is_fake(b)
    assert b.device.type == "cuda"


@requires_no_gpu
def test_device_arg_honored_for_factories() -> None:
    # Rule 1: factories have a BackendSelect kernel, so their `device`
    # argument names the output device.
    with fake_mode(fake_cuda=True):
        a = torch.zeros([3], device="cuda")
    assert a.device.type == "cuda"


@requires_no_gpu
def test_device_arg_honored_via_tensor_options_pack() -> None:
    # Rule 2: _to_copy (what `.to("cuda")` lowers to) carries a
    # dtype/layout/device/pin_memory TensorOptions pack, so its device
    # argument names the output device. (The Python-level `.to()` wrapper
    # itself eagerly initializes the target device before dispatch and
    # cannot run on a GPU-less box — call the op directly.)
    with fake_mode(fake_cuda=True):
        c = torch.ones([3])
        d = torch.ops.aten._to_copy(c, device="cuda")
    assert is_fake(d)
    assert d.device.type == "cuda"


@requires_no_gpu
def test_output_follows_first_tensor_device() -> None:
    # Rule 3: no device argument -> the common tensor-arg device.
    with fake_mode(fake_cuda=True):
        a = torch.ones([2, 2], device="cuda")
        b = a.sum()
    assert b.device.type == "cuda"
