# Drop-in proof for the `torchdistx` alias package: every public name that
# reference-era user code imports from `torchdistx.fake` and
# `torchdistx.deferred_init` is the very object torchdistx_amd defines, so
# whatever tests/test_fake.py and tests/test_deferred_init.py establish for
# torchdistx_amd holds, by identity, for code written against the alias.

import importlib

_PUBLIC_API = {
    "fake": ("fake_mode", "is_fake", "meta_like"),
    "deferred_init": (
        "deferred_init",
        "is_deferred",
        "materialize_module",
        "materialize_tensor",
    ),
}


def test_alias_exports_are_the_native_objects() -> None:
    import torchdistx

    for submodule, names in _PUBLIC_API.items():
        alias = importlib.import_module("torchdistx." + submodule)
        native = importlib.import_module("torchdistx_amd." + submodule)
        assert getattr(torchdistx, submodule) is alias

        for name in names:
            assert getattr(alias, name) is getattr(native, name), name

        # Nothing public in the alias is a re-implementation or a wrapper.
        extra = [
            n for n, v in vars(alias).items()
            if not n.startswith("_") and getattr(native, n, None) is not v
        ]
        assert not extra, (submodule, extra)
