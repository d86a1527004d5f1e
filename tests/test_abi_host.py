"""The ctypes binding is derived from include/*.h (geoformer_amd/_abi.py).  Checked here without a GPU: every struct
layout against a C compiler's sizeof / offsetof, the parsed signatures against expectations written by hand from the
header text, the parser's refusal of what it does not understand, and the constants."""
import ctypes
import os
import re
import shutil
import subprocess
from ctypes import c_char_p, c_double, c_float, c_int, c_longlong, c_size_t, c_uint, c_ulonglong, c_void_p

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
P, I, F = c_void_p, c_int, c_float


def _header(name="geoformer_hip.h"):
    with open(os.path.join(INC, name)) as f:
        return f.read()


def _c_compiler():
    """cc, else the clang that ships beside hipcc (as C); None only when the machine has no C compiler at all."""
    from geoformer_amd import _build

    cc = shutil.which("cc")
    if cc:
        return [cc]
    try:
        beside = os.path.dirname(os.path.realpath(_build._hipcc()))
    except RuntimeError:
        return None
    for name in ("amdclang", "clang"):
        if os.path.exists(os.path.join(beside, name)):
            return [os.path.join(beside, name), "-x", "c"]
    return None


def test_struct_layouts_match_the_c_compiler(tmp_path):
    from geoformer_amd import _abi

    cc = _c_compiler()
    if cc is None:
        pytest.skip("no C compiler on this machine")
    names = re.findall(r"^\}\s*(Gf\w+)\s*;", _header(), re.M)  # every typedef struct of the header, by its own regex
    assert len(names) == 7 + 12 and not re.search(r"typedef\s+struct", _header("geoformer_hip_dev.h"))
    want, lines = {}, ['#include <stddef.h>', '#include <stdio.h>', '#include "geoformer_hip_dev.h"', "int main(void) {"]
    for s in names:
        cls = _abi.struct(s)
        assert cls is _abi.struct(s)  # one class per process
        want[s, ""] = ctypes.sizeof(cls)
        lines.append(f'    printf("{s}  %zu\\n", sizeof({s}));')
        for f, _ in cls._fields_:
            want[s, f] = getattr(cls, f).offset
            lines.append(f'    printf("{s} {f} %zu\\n", offsetof({s}, {f}));')
    lines += ["    return 0;", "}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "probe"
    subprocess.run([*cc, "-std=c99", f"-I{INC}", str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    got = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        s, f, v = re.fullmatch(r"(\w+) (\w*) (\d+)", line).groups()
        got[s, f] = int(v)
    assert len(got) == len(want) > 100
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    sizes = {s: got[s, ""] for s in names}
    assert sizes == {"GfTrainOp": 112, "GfTrainLevel": 88, "GfResBlockParams": 56, "GfUnetLevelParams": 288,
                     "GfUnetParams": 2336, "GfFeederJob": 584, "GfAugBatch": 280,
                     # the rows of the scene tables (8 bytes per column) and of the kernels' output tables
                     "GfPropScene": 48, "GfNmsScene": 64, "GfLblScene": 96, "GfLblRowI": 20, "GfLblRowF": 40,
                     "GfSegScene": 32, "GfMspRow": 20, "GfTileScene": 56, "GfTileScore": 16, "GfBox": 80,
                     "GfBoxScene": 64, "GfBoxIouScene": 40}


# written by hand from the header text (not produced by the parser), compared by ctypes class identity
EXPECTED = {
    "gf_abi_version": (I, []),
    "gf_last_error": (c_char_p, []),
    "gf_host_wait_word": (I, [P, I, c_longlong]),  # const volatile int32_t*, int, long long
    "gf_aug_transform": (I, [P, I, I, c_double, I, P]),
    "gf_aug_draw": (I, [P, c_ulonglong, c_longlong, I, P]),
    "gf_decoder_pre_train_fwd": (I, [P, P, I, I, P, F, c_uint, I, P, P, P, P]),  # float p, unsigned seed
    "gf_unet_fwd": (I, [P, P, P, I, I, I, I, I, P, c_size_t, P, P, P, P]),  # const GfUnetParams*, size_t ws_bytes
    "gf_unet_fwd_phased": (I, [P, P, P, I, I, I, I, I, P, c_size_t, P, P, P, P, P, I, P, P]),  # GfUnetBetween between
    "gf_fg_select": (I, [P, I, I, I, I, P, P, P, P, I] + [P] * 9),  # three header lines
    "gf_index_scratch_bytes": (c_size_t, [c_size_t]),
    "gf_decoder_pre_grad_floats": (c_longlong, []),
    "gf_knn_error_flag": (P, [P, I]),  # returns const int32_t*
    "gf_fps_error_flag": (P, [P, I]),  # the same shape
    "gf_feeder_create": (P, [I]),  # returns void*
    "gf_unet_train_bwd": (I, [P, I, I, P, P, P, P, P, P, P, P]),  # float* const*, float**, unsigned char*
    "gf_proposal_stats_batched": (I, [P, I, I, P, P, c_longlong, I, F, F, I, I, P, P, P, P, P]),
    # include/geoformer_hip_dev.h
    "gf_dev_host_wait_ns": (c_ulonglong, [I]),
    "gf_dev_event_create": (P, []),
    "gf_dev_conv_knobs": (I, [I, I, I, I, I]),
    "gf_dev_fps_plan": (I, [I, P, P, P, P, P]),  # int n, five int* outputs
    "gf_dev_point_grid_plan": (I, [I, P, P, P, P]),  # int n, four int* outputs
}


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_parsed_signature(name):
    from geoformer_amd import _abi

    res, args = _abi.functions()[name]
    assert res is EXPECTED[name][0]
    assert len(args) == len(EXPECTED[name][1]) and all(a is b for a, b in zip(args, EXPECTED[name][1]))


def test_header_facts_the_expectations_rest_on():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert len(re.findall(r"\bgf_host_wait_word\s*\(", text)) == 1
    assert "int gf_host_wait_word(const volatile int32_t* word, int pending, long long timeout_us);" in text
    assert re.search(r"^int gf_fg_select\([^;)]*\n[^;)]*\n[^;)]*\);$", text, re.M)  # a prototype over three lines
    assert "typedef int (*GfUnetBetween)(" in text and "GfUnetBetween between, void* user);" in text
    assert "gf_dev_host_wait_ns" not in text and "gf_dev_host_wait_ns" in _header("geoformer_hip_dev.h")


def test_module_level_names_are_the_header_structs():
    from geoformer_amd import _abi, _lib, unet_exec, unet_train

    assert _lib.FeederJob is _abi.struct("GfFeederJob") and _lib.AugBatch is _abi.struct("GfAugBatch")
    assert unet_exec.UnetParams is _abi.struct("GfUnetParams") and unet_train.TrainOp is _abi.struct("GfTrainOp")
    lv = unet_exec.UnetParams().level
    assert len(lv) == unet_exec.MAX_LEVELS == 8 and isinstance(lv[0], unet_exec.LevelParams)
    assert isinstance(lv[0].blocks[1], unet_exec.ResBlockParams) and len(_lib.FeederJob().bytes) == 16
    assert dict(unet_train.TrainOp._fields_)["gamma"] is c_void_p and dict(unet_train.TrainOp._fields_)["eps"] is c_float
    assert dict(_lib.AugBatch._fields_)["cells"] is c_longlong * 2


@pytest.mark.parametrize("text", [
    "int gf_good(int a);\nint gf_bad(gf_handle h, int n);\n",                # unknown by-value parameter type
    "short gf_bad(int a);\n",                                                  # unknown return type
    "int gf_good(int a);\nint gf_bad(int a, float b;\nint gf_next(int c);\n",  # malformed declaration
    "int gf_bad(int);\n",                                                      # unnamed parameter
    "int gf_good(int a);\nstatic int helper(int a);\n",                        # not a gf_* prototype
    "int gf_twice(int a);\nint gf_twice(int a);\n",
    "typedef struct { int a; wchar_t w; } GfBad;\n",                           # unknown member type
    "typedef struct { int a; int b[GF_NOT_DEFINED]; } GfBad;\n",
    "typedef struct { int a; int (*cb)(int); } GfBad;\n",                      # member that does not parse
])
def test_parser_refuses_what_it_does_not_understand(text):
    from geoformer_amd import _abi
    from geoformer_amd._lib import GeoFormerHipError

    with pytest.raises(GeoFormerHipError, match=r"^probe\.h:[123]: "):
        _abi.parse(text, "probe.h")


def test_parser_names_the_header_line():
    from geoformer_amd import _abi
    from geoformer_amd._lib import GeoFormerHipError

    text = "/* two\n * lines */\n#define GF_N 3\nint gf_good(const float* x, int n);\n\nint gf_bad(half h);\n"
    with pytest.raises(GeoFormerHipError, match=r"^probe\.h:6: gf_bad: unknown parameter type in 'half h'"):
        _abi.parse(text, "probe.h")
    ok = _abi.parse(text.replace("half", "double"), "probe.h")
    assert ok.functions == {"gf_good": (I, [P, I]), "gf_bad": (I, [c_double])} and ok.consts == {"GF_N": 3}
    with pytest.raises(GeoFormerHipError):
        _abi.const("GF_NO_SUCH_CONSTANT")
    with pytest.raises(GeoFormerHipError):
        _abi.struct("GfNoSuchStruct")


def test_every_integer_define_is_a_constant():
    from geoformer_amd import _abi

    found = {}
    for h in ("geoformer_hip.h", "geoformer_hip_dev.h"):
        found.update(re.findall(r"^#define (GF_\w+) (\d+)\b", _header(h), re.M))
    assert len(found) == 17 and found["GF_ABI_VERSION"] == "7"
    for name, value in found.items():
        assert _abi.const(name) == int(value), name
