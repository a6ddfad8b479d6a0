"""CPU: the ctypes binding is derived from include/orp_hip.h (`_lib.parse_header`): the parser on small header texts, every derived
struct against the host C compiler's layout, and no second copy of a signature or a struct left in the package."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from orientedreppoints_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP, I = ctypes.c_void_p, ctypes.c_int


def _sig(text):
    sigs, _, _ = _lib.parse_header(text)
    assert len(sigs) == 1
    return next(iter(sigs.values()))


def test_pointer_arguments_are_void_pointers():
    assert _sig("int f(const float* a, const float* const* b, void* c, float* const* d, const void* e, uint8_t *g);") == (I, [VP] * 6)


def test_integer_widths():
    res, args = _sig("size_t f(long a, long long b, size_t c, int64_t d, int32_t e, uint32_t g, int h, float x, double y);")
    assert res is ctypes.c_size_t
    assert args == [ctypes.c_long, ctypes.c_longlong, ctypes.c_size_t, ctypes.c_longlong, I, ctypes.c_uint32, I, ctypes.c_float,
                    ctypes.c_double]
    assert ctypes.sizeof(args[0]) == ctypes.sizeof(ctypes.c_long) and ctypes.sizeof(args[1]) == 8


def test_void_parameter_list_and_returns():
    assert _sig("int f(void);") == (I, [])
    assert _sig("const char* version(void);") == (ctypes.c_char_p, [])
    assert _sig("char* name(int i);") == (ctypes.c_char_p, [I])
    assert _sig("void g(int* out_host, int n);") == (None, [VP, I])


def test_prototype_over_three_lines_with_comments():
    text = """
    #ifdef __cplusplus
    extern "C" {
    #endif
    /* a block comment with a fake prototype: int not_this(int a); */
    int orp_f(const float* x,   /* the input; with a semicolon */
              long n,           // how many
              void* stream      /* hipStream_t */ );
    #ifdef __cplusplus
    }
    #endif
    """
    sigs, structs, consts = _lib.parse_header(text)
    assert sigs == {"orp_f": (I, [VP, ctypes.c_long, VP])} and not structs and not consts


def test_struct_fields():
    text = """
    typedef struct { float* a; float* b; } orp_inner;
    typedef struct orp_outer_tag {
      const float* data;          /* c_void_p */
      int m0, n, flip;            /* a comma list */
      int32_t reserved[2];
      double scale;
      const orp_inner* levels;    /* pointer to a parsed struct */
      const void* const* table;
    } orp_outer;
    int use(const orp_outer* o, int n);
    """
    sigs, structs, _ = _lib.parse_header(text)
    inner, outer = structs["orp_inner"], structs["orp_outer"]
    assert issubclass(outer, ctypes.Structure) and list(structs) == ["orp_inner", "orp_outer"]
    assert [n for n, _ in outer._fields_] == ["data", "m0", "n", "flip", "reserved", "scale", "levels", "table"]
    types = dict(outer._fields_)
    assert types["data"] is VP and types["table"] is VP and types["m0"] is I and types["flip"] is I and types["scale"] is ctypes.c_double
    assert types["reserved"]._type_ is I and types["reserved"]._length_ == 2
    assert types["levels"] is ctypes.POINTER(inner)
    assert [getattr(outer, n).offset for n, _ in outer._fields_] == [0, 8, 12, 16, 20, 32, 40, 48] and ctypes.sizeof(outer) == 56
    assert sigs["use"] == (I, [VP, I])          # a struct pointer as an ARGUMENT stays a plain address


def test_constants():
    text = "#ifndef ORP_X_H_\n#define ORP_X_H_\n#define ORP_OK 0\n#define ORP_EINVAL (-1)  /* bad */\n# define ORP_BIG ( -131072 )\n" \
           "#define ORP_HEX 0x10\n#define OTHER 5\n#endif\n"
    assert _lib.parse_header(text)[2] == {"ORP_OK": 0, "ORP_EINVAL": -1, "ORP_BIG": -131072, "ORP_HEX": 16}


@pytest.mark.parametrize("text, named", [
    ("int f(half_t x);", "half_t"),                                         # unknown scalar
    ("int f(const half_t* x);", "half_t"),                                  # unknown pointee
    ("unsigned f(int x);", "unsigned"),                                     # unknown result
    ("float* f(int x);", "float*"),                                         # a pointer result other than char*
    ("int f(int (*cb)(int), void* stream);", "cb"),                         # function-pointer argument
    ("int f(int);", "f(int)"),                                              # unnamed argument
    ("int f(long long);", "f(long long)"),
    ("int f(int a[4]);", "a[4]"),
    ("int f();", "f()"),
    ("typedef struct { int a : 3; int b; } orp_bits;", "a : 3"),            # bit-field
    ("typedef struct { half_t a; } orp_s;", "half_t"),
    ("typedef struct { float *a, *b; } orp_s;", "*b"),
    ("typedef struct { void (*cb)(void); } orp_s;", "cb"),
    ("typedef struct { struct { int a; } in; } orp_s;", "struct"),          # nested struct
    ("typedef int orp_int;", "orp_int"),
    ("int f(int a)", "f(int a)"),                                           # no semicolon
    ("int f(int a);\nint f(int a, int b);", "int f(int a, int b)"),         # one name, two prototypes
    ("#define ORP_N (1 << 4)\n", "ORP_N"),
    ("#define ORP_N 3.5\n", "ORP_N"),
])
def test_unmappable_declarations_raise(text, named):
    with pytest.raises(_lib.OrpHipError) as e:
        _lib.parse_header(text)
    assert named in str(e.value), str(e.value)


def test_missing_header_is_named(monkeypatch):
    monkeypatch.setattr(_lib, "HEADER_PATH", os.path.join(ROOT, "include", "no_such_header.h"))
    with pytest.raises(_lib.OrpHipError, match="no_such_header.h"):
        _lib._load_header()


STRUCT_SIZES = {"orp_dcn_level": 32, "orp_dcn_heads": 56, "orp_train_image_desc": 64, "orp_pp_view": 56, "orp_level_desc": 32,
                "orp_norm_level": 24, "orp_bias_level": 40, "orp_conv_level": 40, "orp_wgrad_level": 24, "orp_dcn_bwd_level": 48,
                "orp_dcn_head_level": 24, "orp_dcn_level_h": 32}


def test_struct_layouts_match_the_c_compiler(tmp_path):
    """sizeof and every offsetof, as the host C compiler lays include/orp_hip.h out, against the derived ctypes classes."""
    assert sorted(_lib._STRUCTS) == sorted(STRUCT_SIZES)
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler (cc / gcc / clang) on PATH")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "orp_hip.h"', 'int main(void) {']
    for name, cls in _lib._STRUCTS.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        for field, _ in cls._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, field, name, field))
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines + ["  return 0;", "}"]) + "\n")
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    want = dict((k, int(v)) for k, v in (l.split() for l in out.splitlines()))
    got = {}
    for name, cls in _lib._STRUCTS.items():
        got[name] = ctypes.sizeof(cls)
        got.update({"%s.%s" % (name, f): getattr(cls, f).offset for f, _ in cls._fields_})
    assert got == want
    assert {n: want[n] for n in STRUCT_SIZES} == STRUCT_SIZES


def test_op_modules_bind_the_derived_structs():
    import importlib
    import numpy as np
    ops = {n: importlib.import_module("orientedreppoints_amd.mmdet_ops." + n)
           for n in ("fused_norm", "deform_conv", "deform_conv_backward", "train_ops", "train_image_ops")}
    core = importlib.import_module("orientedreppoints_amd.mmdet_models.core")
    bound = {"orp_norm_level": ops["fused_norm"]._NormLevel, "orp_bias_level": ops["fused_norm"]._BiasLevel,
             "orp_conv_level": ops["fused_norm"]._ConvLevel, "orp_wgrad_level": ops["fused_norm"]._WgradLevel,
             "orp_dcn_level": ops["deform_conv"]._DcnLevel, "orp_dcn_head_level": ops["deform_conv"]._DcnHeadLevel,
             "orp_dcn_heads": ops["deform_conv"]._DcnHeads, "orp_dcn_bwd_level": ops["deform_conv_backward"]._BwdLevel,
             "orp_level_desc": ops["train_ops"]._LevelDesc, "orp_pp_view": core.PpView}
    for name, cls in bound.items():
        assert cls is _lib.struct(name), name
    assert dict(_lib.struct("orp_dcn_heads")._fields_)["levels"] is ctypes.POINTER(_lib.struct("orp_dcn_head_level"))
    desc = ops["train_image_ops"].DESC_DTYPE
    assert desc == np.dtype(_lib.struct("orp_train_image_desc")) and desc.itemsize == 64
    assert desc.names == ("src_offset", "scratch_offset", "src_h", "src_w", "new_h", "new_w", "pad_h", "pad_w", "flip", "rotate",
                          "x_table", "y_table", "reserved")
    assert desc["src_offset"] == np.dtype("<i8") and desc["src_h"] == np.dtype("<i4") and desc["reserved"].shape == (2,)


def test_package_writes_no_struct_fields():
    pkg = os.path.join(ROOT, "orientedreppoints_amd")
    seen = 0
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                seen += 1
                src = open(os.path.join(dp, f), errors="replace").read()
                assert not re.search(r"_fields_\s*(=|\+=)|\._fields_\b.*\bappend|\._fields_\b.*\bextend", src), os.path.join(dp, f)
    assert seen > 20


def test_signature_table_is_the_headers():
    text = re.sub(r"/\*.*?\*/", " ", open(_lib.HEADER_PATH).read(), flags=re.S)
    text = re.sub(r"typedef struct[^{}]*\{[^{}]*\}[^;]*;", " ", text)
    prototypes = re.findall(r"\b(\w+)\s*\([^()]*\)\s*;", text)
    assert len(prototypes) == len(set(prototypes)) == len(_lib._SIGNATURES) == len(_lib.parse_header(open(_lib.HEADER_PATH).read())[0])
    assert sorted(prototypes) == sorted(_lib._SIGNATURES)
    for name, value in _lib._SIGNATURES.items():
        assert isinstance(value, tuple) and len(value) == 2 and isinstance(value[1], list), name
        res, args = value
        assert res is None or res is ctypes.c_char_p or res in _lib._SCALARS.values(), name
        assert all(a is VP or a in _lib._SCALARS.values() for a in args), name
    assert (_lib.ORP_OK, _lib.ORP_EINVAL, _lib.ORP_EWORKSPACE, _lib.ORP_ETOOBIG, _lib.ORP_NMS_MAX_BOXES) == (0, -1, -2, -3, 131072)
    assert _lib._CONSTANTS["ORP_DCN_BWD_INPUT"] == 1 and _lib._CONSTANTS["ORP_DCN_BWD_SPARSE"] == 2
