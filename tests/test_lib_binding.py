"""CPU: the library handle binds an entry point's prototype when it is first looked up (_lib._Handle), load() still
checks that every declared prototype is exported, and a process does not hold a function object per declaration."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from geoformer_amd import _lib

    return _lib.load()


def test_prototype_is_bound_on_first_lookup_and_cached(lib):
    from geoformer_amd import _abi, _lib

    assert isinstance(lib, _lib._Handle) and isinstance(lib, ctypes.CDLL)
    name = "gf_tile_stitch_max_classes"
    fn = getattr(lib, name)
    res, args = _abi.functions()[name]
    assert fn.restype is res and list(fn.argtypes) == list(args)
    assert name in vars(lib) and getattr(lib, name) is fn  # an attribute of the handle from now on
    fn = lib.gf_tile_stitch_scores
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 11
    assert _lib.EXPORTS is _abi.functions()


def test_missing_symbols_are_attribute_errors(lib):
    from geoformer_amd import _lib

    with pytest.raises(AttributeError):
        lib.gf_no_such_entry_point
    assert not hasattr(lib, "gf_no_such_entry_point")

    class Exports:  # a library that lacks one declared entry point
        def __getitem__(self, name):
            if name == "gf_tile_stitch_scores":
                raise AttributeError(name)
            return None

    with pytest.raises(AttributeError, match="gf_tile_stitch_scores"):
        _lib._declare(Exports())


def test_a_function_is_on_the_handle_only_with_its_prototype():
    """The function object becomes an attribute of the handle after its argtypes are set, never before: every
    attribute assignment of the handle is watched."""
    from geoformer_amd import _abi, _lib

    seen = []

    class Watched(_lib._Handle):
        def __setattr__(self, name, value):
            if name.startswith("gf_"):
                seen.append((name, value.restype, value.argtypes))
            super().__setattr__(name, value)

    h = Watched(_lib.LIB_PATH)
    names = list(_abi.functions())
    for name in names:
        getattr(h, name)
    assert [n for n, _, _ in seen] == names
    for name, res, args in seen:
        want_res, want_args = _abi.functions()[name]
        assert res is want_res and args is not None and list(args) == list(want_args), name


def test_concurrent_first_lookups_never_see_an_unbound_function():
    """Eight threads look the same names up on a cold handle while a ninth reads the handle's attributes as they
    appear: whatever any of them gets has its prototype (no sleeping: the threads run until every name is bound)."""
    import threading

    from geoformer_amd import _abi, _lib

    names = [n for n, (_, a) in _abi.functions().items() if a]  # the entry points that take arguments
    bad, done = [], threading.Event()
    for _ in range(5):
        h = _lib._Handle(_lib.LIB_PATH)
        start = threading.Barrier(9)
        done.clear()

        def lookups():
            start.wait()
            for name in names:
                if getattr(h, name).argtypes is None:
                    bad.append(name)

        def reader():
            start.wait()
            while not done.is_set():
                for name, fn in list(vars(h).items()):
                    if name.startswith("gf_") and fn.argtypes is None:
                        bad.append(name)

        threads = [threading.Thread(target=lookups) for _ in range(8)]
        watcher = threading.Thread(target=reader)
        for t in threads + [watcher]:
            t.start()
        for t in threads:
            t.join()
        done.set()
        watcher.join()
        assert all(n in vars(h) for n in names)
    assert not bad, sorted(set(bad))


def test_load_keeps_no_function_object_per_declaration():
    """A fresh handle holds none of the declared entry points until one is looked up."""
    from geoformer_amd import _abi, _lib

    fresh = _lib._Handle(_lib.LIB_PATH)
    _lib._declare(fresh)
    assert not [n for n in _abi.functions() if n in vars(fresh)]
    assert fresh.gf_abi_version() == _abi.const("GF_ABI_VERSION") and "gf_abi_version" in vars(fresh)
