"""The C-ABI library loads and exports exactly the entry points include/speakerguard_hip.h declares.
CPU only: no compute call is made (hipcc cross-compiles gfx950 without a GPU)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from speakerguard_amd import _native


def header_text():
    """include/speakerguard_hip.h without its comments"""
    text = open(os.path.join(ROOT, "include", "speakerguard_hip.h")).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def header_functions():
    return sorted(set(re.findall(r"\b(sg_[a-z0-9_]+)\s*\(", header_text())))


# ---------------------------------------------------------------- the prototypes against the ctypes mirror (_native.load's table)
_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64,
            "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "double": ctypes.c_double}
_STRUCTS = {"sg_loss_spec": _native.LossSpec, "sg_dither": _native.Dither, "sg_pgd_params": _native.PgdParams,
            "sg_xv_weights": _native.XvWeights, "sg_an_weights": _native.AnWeights, "sg_feco_params": _native.FecoParams,
            "sg_wav_defense": _native.WavDefense, "sg_wav_filter": _native.WavFilter, "sg_wav_stage": _native.WavStage}
# what a typed pointer of the mirror may point to, by the C type behind the `*` (anything else: c_void_p only)
_POINTEES = dict(_SCALARS, **_STRUCTS, **{"sg_ctx*": ctypes.c_void_p})
_RETURNS = dict(_SCALARS, **{"void": None, "const char*": ctypes.c_char_p})


def declared(name):
    """(return type, [parameter types]) of `name` as the header spells them: ``const`` kept on the return type only, the
    parameters' names and ``const`` dropped, ``*`` attached to the type"""
    m = re.search(r"^\s*([A-Za-z_][\w \t\*]*?)\s*\b%s\s*\(([^)]*)\)\s*;" % name, header_text(), flags=re.M)
    assert m, "%s is not declared" % name
    params = []
    for param in m.group(2).split(","):
        param = " ".join(param.replace("*", " * ").split())
        if param in ("", "void"):
            continue
        words = [w for w in param.split()[:-1] if w != "const"]  # drop the parameter's name
        params.append(words[0] + "".join(words[1:]))
        assert set(words[1:]) <= {"*"} and re.fullmatch(r"\w+", param.split()[-1]), param
    return " ".join(m.group(1).replace("*", " * ").split()).replace(" *", "*"), params


def declared_argtypes(name):
    """the mirror `name`'s prototype asks for, with every struct pointer typed and every other pointer a ``c_void_p``"""
    return [_SCALARS[t] if t in _SCALARS else ctypes.POINTER(_STRUCTS[t[:-1]]) if t[:-1] in _STRUCTS else ctypes.c_void_p
            for t in declared(name)[1] if t in _SCALARS or t.endswith("*")]


@pytest.mark.parametrize("name", _native.EXPORTS)
def test_binding_mirrors_the_prototype(name):
    """arity; every scalar exactly; a pointer as ``c_void_p`` or as ``POINTER`` of the mirrored struct / scalar it points to;
    the return type"""
    ret, params = declared(name)
    fn = getattr(_native.load(), name)
    assert fn.restype is _RETURNS[ret], (name, ret, fn.restype)
    assert fn.argtypes is not None and len(fn.argtypes) == len(params), (name, len(fn.argtypes or ()), params)
    for i, (have, want) in enumerate(zip(fn.argtypes, params)):
        if want.endswith("*"):
            typed = _POINTEES.get(want[:-1])
            assert have is ctypes.c_void_p or (typed is not None and have is ctypes.POINTER(typed)), (name, i, want, have)
        else:
            assert have is _SCALARS[want], (name, i, want, have)  # (a type this table does not know is a KeyError: add it)


def test_library_exports_every_declared_symbol():
    assert os.path.exists(_native.LIB_PATH), "run `make` (or __graft_entry__.build()) first"
    lib = ctypes.CDLL(_native.LIB_PATH)
    names = header_functions()
    assert len(names) >= 15
    for n in names:
        assert hasattr(lib, n), "missing export %s" % n
    assert sorted(_native.EXPORTS) == names, "python binding list and header disagree"


def test_version_and_loader():
    lib = _native.load()
    assert lib.sg_version() == 100
    assert lib.sg_xv_num_frames(48000) == 300
    assert lib.sg_xv_num_frames(52960) == 331
    assert lib.sg_xv_num_frames(100) == 0


def test_struct_layouts_match_header(tmp_path):
    """sizeof of every struct that crosses the boundary, as gcc lays out the header's definition (x86-64 SysV), against
    the ctypes mirror: catches field-order / padding drift."""
    import subprocess
    pairs = sorted(_STRUCTS.items())
    assert len(pairs) == 9
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "speakerguard_hip.h"\nint main(void) {\n' +
                   "".join('    printf("%%zu\\n", sizeof(%s));\n' % c for c, _ in pairs) + "    return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    for (cname, ctype), size in zip(pairs, sizes):
        assert ctypes.sizeof(ctype) == size, (cname, ctypes.sizeof(ctype), size)
    assert ctypes.sizeof(_native.LossSpec) == 32 and ctypes.sizeof(_native.Dither) == 48


def test_gradient_buffer_ids_match_the_header():
    """``_native.SG_GRAD`` (the names ``xv_plda.read_gradient`` takes) against the SG_GRAD_* of sg_xv_debug_gradient"""
    ids = {k: int(v) for k, v in re.findall(r"#define\s+SG_GRAD_(\w+)\s+(\d+)", header_text())}
    assert ids == {"DEMB": 0, "DACT1": 1, "DSTATS": 6, "DFEATS": 7, "DFEATS_RAW": 8}
    want = {"demb": ids["DEMB"], "dstats": ids["DSTATS"], "dfeats": ids["DFEATS"], "dfeats_raw": ids["DFEATS_RAW"]}
    want.update({"dact%d" % l: ids["DACT1"] + l - 1 for l in range(1, 6)})
    assert _native.SG_GRAD == want
    assert "sg_xv_debug_gradient" in _native.EXPORTS and declared("sg_xv_debug_gradient")[1][-2:] == ["int32_t*", "void*"]


def test_audionet_gradient_buffer_ids_match_the_header():
    """``_native.SG_AN_GRAD`` (the names ``audionet_csine.read_gradient`` takes) against the SG_AN_GRAD_* of sg_an_debug_gradient"""
    ids = {k: int(v) for k, v in re.findall(r"#define\s+SG_AN_GRAD_(\w+)\s+(\d+)", header_text())}
    assert ids == {"DACT1": 0, "DPOOL1": 7, "DPOOL4": 8, "DPOOL6": 9, "DPRE": 10, "PRE": 11, "ACT1_UNPOOLED": 12,
                   "ACT4_UNPOOLED": 13, "ACT6_UNPOOLED": 14}
    want = {k.lower(): v for k, v in ids.items() if k != "DACT1"}
    want.update({"dact%d" % l: ids["DACT1"] + l - 1 for l in range(1, 8)})  # conv2 .. conv8
    assert _native.SG_AN_GRAD == want and sorted(want.values()) == list(range(15))
    assert "sg_an_debug_gradient" in _native.EXPORTS and declared("sg_an_debug_gradient")[1][-2:] == ["int32_t*", "void*"]


def test_missing_library_is_loud(monkeypatch, tmp_path):
    monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.setattr(_native, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_native.NativeError):
        _native.load()


def test_model_refuses_cpu_device():
    from speakerguard_amd import synth
    from speakerguard_amd.model.xv_plda import xv_plda
    with pytest.raises(_native.NativeError):
        xv_plda.from_weights(synth.make_xv_weights(), device="cpu")


def test_header_is_plain_c(tmp_path):
    """The drop-in boundary is a C ABI: include/speakerguard_hip.h must compile as C99 on its own."""
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "hdr.c"
    src.write_text('#include "speakerguard_hip.h"\nint use(void) { return sg_version(); }\n')
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(root, "include"),
                        "-c", str(src), "-o", str(tmp_path / "hdr.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
