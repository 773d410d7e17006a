"""CPU-side checks of the C-ABI: include/svolsdf_hip.h stands alone as C and C++, the library builds for gfx950 against it,
loads, and exports exactly what it declares, and the ctypes table svs_hip/lib.py derives from it is the one its rules
promise (no compute calls)."""
import ctypes
import os
import re
import shutil
import subprocess
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_longlong, c_size_t, c_void_p

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "svolsdf_hip.h")
_P, _PP = c_void_p, POINTER(c_void_p)


def _build_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("svs_build", os.path.join(ROOT, "s-volsdf_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def lib():
    _build_module().build(verbose=False)
    from svs_hip import lib as L
    return L


def _llvm_tool(name):
    """A tool of the LLVM toolchain the library was built with: the one hipcc belongs to."""
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(shutil.which(_build_module()._hipcc()))))
    for d in (os.path.join(rocm, "lib", "llvm", "bin"), os.path.join(rocm, "llvm", "bin")):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    raise AssertionError(f"{name} not found under {rocm}")


def _header_decls():
    """Name -> argument count by a regular expression of this file's own (no code shared with the binding's parser)."""
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decls = {}
    for m in re.finditer(r"\b(?:int|size_t|const char\*)\s+(svs_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        args = m.group(2).strip()
        decls[m.group(1)] = 0 if args in ("void", "") else len([a for a in args.split(",") if a.strip()])
    return decls


def test_header_matches_library_and_ctypes_table(lib):
    """The header's functions = the library's dynamic svs_ symbols = the derived table, and load() has set that table's
    types on every one of them."""
    decls = _header_decls()
    L = lib.load()
    assert set(decls) == set(lib.SIGNATURES), set(decls) ^ set(lib.SIGNATURES)
    out = subprocess.run([_llvm_tool("llvm-readelf"), "--dyn-syms", "--wide", lib.LIB_PATH], check=True, capture_output=True,
                         text=True).stdout
    exported = {f[7].split("@")[0] for f in (line.split() for line in out.splitlines())
                if len(f) == 8 and f[6] != "UND" and f[7].startswith("svs_")}
    assert exported == set(lib.SIGNATURES), exported ^ set(lib.SIGNATURES)
    for name, nargs in decls.items():
        assert hasattr(L, name), f"{name} declared in the header but not exported"
        res, args = lib.SIGNATURES[name]
        assert len(args) == nargs, name
        fn = getattr(L, name)
        assert fn.restype is res, name
        assert len(fn.argtypes) == nargs and all(a is b for a, b in zip(fn.argtypes, args)), name
    assert L.svs_version() == lib.ABI_VERSION == 101


def test_parser_rules_on_header_snippets(lib):
    """Every rule of the binding's header parser on literal C text, and its refusal of what it cannot classify."""
    consts, structs, sigs = lib.parse_header("""
        #ifndef X_H
        #define X_H
        #include <stddef.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define SVS_HOST
        #define SVS_ABI_VERSION 7
        #define SVS_EBAD (-9)   /* with a comment */
        enum { SVS_A = 0, SVS_B = 2 };
        /* a declaration
         * spread over three lines */
        int svs_three(const float* x, int n,
                      float scale,   // one per line
                      void* hip_stream);
        int svs_none(void);
        const char* svs_text(void);
        size_t svs_bytes(size_t n, double d, long long k);
        int svs_tables(const float* const* unmarked, const float* const SVS_HOST* marked, void* SVS_HOST* out,
                       void* const SVS_HOST* in);
        int svs_host(unsigned char* state, const long long SVS_HOST* ranks, const float SVS_HOST* f,
                     double SVS_HOST* d, int SVS_HOST* i, char* buf, const char* name, const uint8_t* const* masks);
        typedef struct svs_job {
          const float *a0, *b0; long long sa0, sb0;
          int n, ldw;
          float* dW;
          size_t bytes; double x; float y;
        } svs_job;
        int svs_jobs(const svs_job* jobs, int n);
        #ifdef __cplusplus
        }
        #endif
        #endif
    """)
    assert consts == {"SVS_ABI_VERSION": 7, "SVS_EBAD": -9, "SVS_A": 0, "SVS_B": 2}
    assert sigs == {
        "svs_three": (c_int, [_P, c_int, c_float, _P]),
        "svs_none": (c_int, []),
        "svs_text": (c_char_p, []),
        "svs_bytes": (c_size_t, [c_size_t, c_double, c_longlong]),
        "svs_tables": (c_int, [_P, _PP, _PP, _PP]),
        "svs_host": (c_int, [_P, POINTER(c_longlong), POINTER(c_float), POINTER(c_double), POINTER(c_int), c_char_p, c_char_p, _P]),
        "svs_jobs": (c_int, [_P, c_int]),
    }
    assert structs == {"svs_job": [("a0", _P), ("b0", _P), ("sa0", c_longlong), ("sb0", c_longlong), ("n", c_int),
                                   ("ldw", c_int), ("dW", _P), ("bytes", c_size_t), ("x", c_double), ("y", c_float)]}
    refused = {
        "int svs_f(const float* x, half y);": "svs_f",                       # a parameter of an unknown type
        "int svs_g(long n);": "svs_g",
        "int svs_h(float SVS_HOST x);": "svs_h",                             # the marker on a value
        "int svs_i(const unsigned char SVS_HOST* s);": "svs_i",              # a host pointer to a type with no rule
        "int svs_j(float*** p);": "svs_j",
        "int svs_k(int (*callback)(int));": "svs_k",
        "short svs_l(int n);": "svs_l",                                      # a return type with no rule
        "typedef struct svs_s { float a[4]; } svs_s;": "svs_s",              # an unparsable struct field
        "typedef struct svs_t { int a : 3; } svs_t;": "svs_t",
        "typedef struct svs_u { struct svs_u* next; } svs_u;": "svs_u",
        "typedef struct svs_v { int a; } svs_w;": "svs_v",
        "#define SVS_MAX(a, b) ((a) > (b) ? (a) : (b))": "SVS_MAX",
        "enum { SVS_C = 1 << 3 };": "SVS_C",
        "static inline int svs_m(int n) { return n; }": "svs_m",
    }
    for text, named in refused.items():
        with pytest.raises(lib.SvsError, match=named):
            lib.parse_header(text)


def test_three_real_signatures(lib):
    """The rules on the real header: the list INTEGRATION.md prints, five doubles and a long long, a pointer table and a
    host float array."""
    assert lib.SIGNATURES["svs_sdf_vals"] == (c_int, [_P, c_int, _P, c_int, _P, _P, c_int, c_int, _P, c_int, c_float, c_float,
                                                      c_int, _P, _P, c_int, c_int, _P])
    assert lib.SIGNATURES["svs_clip_guard_adam"] == (c_int, [_P, _P, _P, _P, c_longlong, c_int, _P, c_double, c_double,
                                                             c_double, c_double, c_double, _P, _P, _P])
    assert lib.SIGNATURES["svs_warp_variance"] == (c_int, [_P, _PP, POINTER(c_float), c_int, c_int, c_int, c_int, c_int, _P, _P,
                                                           c_int, _P])


def test_header_stands_alone(lib, tmp_path):
    """The header compiles as C99 and as C++17 with nothing else on the include path, and the C compiler lays the two job
    structs out as ctypes lays out the classes derived from them."""
    clang = _llvm_tool("clang")
    subprocess.run([clang, "-std=c99", "-x", "c", "-fsyntax-only", "-Wall", "-Werror", HEADER], check=True)
    subprocess.run([clang, "-std=c++17", "-x", "c++", "-fsyntax-only", "-Wall", "-Werror", HEADER], check=True)
    classes = {"svs_wgrad_job": lib.WGradJob, "svs_unpack_job": lib.UnpackJob}
    lines = ['#include <stdio.h>', '#include "svolsdf_hip.h"', "int main(void) {"]
    for c_name, cls in classes.items():
        lines.append(f'  printf("{c_name} %zu\\n", sizeof({c_name}));')
        lines += [f'  printf("{c_name}.{f} %zu\\n", offsetof({c_name}, {f}));' for f, _ in cls._fields_]
    lines += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.run([clang, "-std=c99", "-I", os.path.dirname(HEADER), str(tmp_path / "layout.c"), "-o", exe], check=True)
    got = dict(line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    want = {}
    for c_name, cls in classes.items():
        want[c_name] = str(ctypes.sizeof(cls))
        want.update({f"{c_name}.{f}": str(getattr(cls, f).offset) for f, _ in cls._fields_})
    assert got == want
    assert len(want) == 2 + 17 + 13


def test_size_queries(lib):
    L = lib.load()
    assert L.svs_stream_bytes(1) > L.svs_stream_bytes(0) > 1 << 20
    assert L.svs_stream_bytes(3) > 1 << 20
    assert L.svs_sampler_cap() >= 640 and L.svs_sampler_max_new() == 128
    assert L.svs_sdf_hbuf_bytes(128) == 4 * 8 * 128 * 64 * 4
    assert L.svs_feat_tiles_bytes(129) == 8 * 128 * 64 * 4


def test_argument_errors_are_reported(lib):
    L = lib.load()
    rc = L.svs_rays_from_uv(None, None, None, 0, None, None, None, None)
    assert rc < 0 and b"svs_rays_from_uv" in L.svs_last_error_string()
    rc = L.svs_composite(4, 1000, None, None, None, None, None, None, 0.0, None, None, None, None, None, None)
    assert rc < 0


def test_missing_library_fails_loudly(lib, monkeypatch):
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setattr(lib, "LIB_PATH", "/nonexistent/libsvolsdf_hip.so")
    with pytest.raises(lib.SvsError):
        lib.load()


def test_precision_setting_is_validated(monkeypatch):
    """SVS_MLP_PRECISION names one of the three arithmetic settings (f32 covers the background networks too since round 5:
    csrc/svs_bg_f32.hip); anything else is an error before any device work."""
    import pytest
    from svs_hip import ops
    monkeypatch.setenv("SVS_MLP_PRECISION", "f32")
    assert ops.default_precision() == ops.F32
    monkeypatch.setenv("SVS_MLP_PRECISION", "bf16")
    with pytest.raises(ValueError):
        ops.default_precision()
    # the background entry points refuse a precision they do not know (argument check, nothing is launched)
    import ctypes
    from svs_hip import lib
    L = lib.load()
    d = ctypes.c_void_p(64)
    assert L.svs_bg_sdf_eval(d, 32, d, 7, d, d, None, None, None, None) < 0 and b"precision" in L.svs_last_error_string()
    assert L.svs_bg_rgb_eval(32, d, 0, d, d, 7, d, None, None) < 0 and b"precision" in L.svs_last_error_string()


def test_argument_errors_come_back_as_codes():
    """Entry points validate their arguments before touching the device: null pointers and bad shapes return the
    documented negative codes (and set the error string) -- no GPU needed, nothing is launched."""
    import ctypes
    from svs_hip import lib
    L = lib.load()
    dummy = ctypes.c_void_p(64)                      # never dereferenced: the shape checks come first
    rc = L.svs_featurenet_fpn(None, 512, 640, 8, None, None, None, None, None, None, None)
    assert rc < 0 and b"null" in L.svs_last_error_string()
    rc = L.svs_featurenet_fpn(dummy, 510, 640, 8, dummy, dummy, dummy, dummy, dummy, dummy, None)
    assert rc < 0 and b"multiples of 4" in L.svs_last_error_string()
    assert L.svs_featurenet_fpn_workspace_bytes(8, 512, 640) > 0 and L.svs_featurenet_fpn_workspace_bytes(8, 2, 2) == 0
    rc = L.svs_conv2d(dummy, dummy, None, None, 0, dummy, 8, 8, 16, 16, 4, 1, 0, None)        # k = 4
    assert rc < 0 and b"k in {1,3,5}" in L.svs_last_error_string()
    rc = L.svs_wgrad_multi(None, 0, 1, None)
    assert rc < 0
    rc = L.svs_mesh_sample_count(None, 5, None, None)
    assert rc < 0 and b"svs_mesh_sample_count" in L.svs_last_error_string()
    rc = L.svs_mesh_sample_points(dummy, 5, None, dummy, None)
    assert rc < 0 and b"svs_mesh_sample_points" in L.svs_last_error_string()
    assert L.svs_mesh_sample_count(None, 0, None, None) == 0          # an empty mesh is not an error
    # launch plans and the eikonal points: argument checks come before any HIP call
    plan = ctypes.c_void_p()
    assert L.svs_plan_build(None, None, 0, ctypes.byref(plan)) < 0 and not plan.value
    assert L.svs_plan_build(dummy, None, 2, ctypes.byref(plan)) < 0          # two side streams announced, none given
    assert L.svs_plan_run(None, None) < 0 and L.svs_plan_destroy(None) < 0
    counts = (ctypes.c_int * 8)()
    assert L.svs_plan_info(None, counts) < 0 and L.svs_plan_describe(None, None, 0) < 0
    rc = L.svs_eikonal_points(None, dummy, dummy, dummy, 4, dummy, None)
    assert rc < 0 and b"svs_eikonal_points" in L.svs_last_error_string()
    assert L.svs_eikonal_points(dummy, dummy, dummy, dummy, 0, dummy, None) < 0
    assert L.svs_split_last(dummy, 4, 1, dummy, dummy, None) < 0 and L.svs_split_last(None, 4, 3, dummy, dummy, None) < 0
    assert L.svs_stage_in(None, dummy, 64, None) < 0 and L.svs_stage_in(dummy, dummy, 6, None) < 0
    assert L.svs_stage_in(ctypes.c_void_p(68), dummy, 64, None) < 0            # not 16-byte aligned


def test_composite_entry_points_validate_sample_counts():
    """The four compositing entry points share one argument check: sample counts outside what the kernels hold and a normal
    map without normals come back with the documented codes and messages (dummy pointers, nothing is launched)."""
    import ctypes
    from svs_hip import lib
    L = lib.load()
    d = ctypes.c_void_p(64)
    EINVAL, ESHAPE = -1, -2
    calls = {
        "svs_composite": lambda S, Nb, normals=d: L.svs_composite(4, S, d, d, d, normals, d, d, 1e-4, d, d, d, d, d, None),
        "svs_composite_bwd": lambda S, Nb: L.svs_composite_bwd(4, S, d, d, d, d, d, 1e-4, d, d, d, d, d, d, d, None),
        "svs_composite_bg": lambda S, Nb, normals=d: L.svs_composite_bg(4, S, Nb, d, d, d, d, normals, d, d, 1e-4, d, d, d, d,
                                                                        d, d, d, d, d, d, d, d, None),
        "svs_composite_bg_bwd": lambda S, Nb: L.svs_composite_bg_bwd(4, S, Nb, d, d, d, d, d, d, 1e-4, d, d, d, d, d, d, d, d,
                                                                     d, d, d, d, d, d, None),
    }
    for name in ("svs_composite", "svs_composite_bwd"):
        for S in (1, 257):
            assert calls[name](S, 0) == ESHAPE
            assert L.svs_last_error_string() == b"%s: n_samples must be in [2,256]" % name.encode()
    for name in ("svs_composite_bg", "svs_composite_bg_bwd"):
        for S, Nb in ((1, 32), (256, 32), (97, 1), (97, 65)):
            assert calls[name](S, Nb) == ESHAPE
            assert L.svs_last_error_string() == b"%s: sample counts out of range" % name.encode()
    for name in ("svs_composite", "svs_composite_bg"):
        assert calls[name](97, 32, normals=None) == EINVAL
        assert L.svs_last_error_string() == b"%s: normal_map needs normals" % name.encode()


def test_fragment_packers_validate_before_any_launch():
    """The four packers of the cost-regularisation U-Net's A fragments accept what the kernel they pack for accepts: a null
    pointer or another (Cin, Cout) is SVS_EINVAL with the entry point named, on a machine without a GPU; their buffers have
    the sizes the queries report."""
    from svs_hip import lib
    L = lib.load()
    EINVAL = -1
    p = 4096                                                       # never dereferenced: the checks come first
    packers = {
        "svs_conv3d_mfma_pack": (lambda w, f, cin, cout: L.svs_conv3d_mfma_pack(w, cin, cout, f, None), (8, 16), [(12, 8), (8, 17), (8, 0), (64, 8)]),
        "svs_conv3d_pair_pack": (lambda w, f, cin, cout: L.svs_conv3d_pair_pack(w, cin, cout, f, None), (32, 8), [(12, 8), (8, 9), (8, 0), (64, 8)]),
        "svs_conv3d_rows_pack": (lambda w, f, cin, cout: L.svs_conv3d_rows_pack(w, cin, cout, f, None), (16, 16), [(8, 16), (32, 16), (16, 17), (16, 0)]),
        "svs_conv3d_s2c8_pack": (lambda w, f, cin, cout: L.svs_conv3d_s2c8_pack(w, cout, f, None), (8, 16), [(8, 17), (8, 0)]),
    }
    for name, (call, good, unsupported) in packers.items():
        for w, f in ((None, p), (p, None)):
            assert call(w, f, *good) == EINVAL, name
            assert L.svs_last_error_string().startswith(name.encode() + b": bad argument")
        for cin, cout in unsupported:
            assert call(p, p, cin, cout) == EINVAL, (name, cin, cout)
            assert L.svs_last_error_string().startswith(name.encode() + b": bad argument")
    # [fragment pairs][2 pieces][64 lanes][16 B]
    assert [L.svs_conv3d_mfma_wfrag_bytes(c) for c in (8, 16, 32)] == [7 * 2048, 14 * 2048, 27 * 2048]
    assert [L.svs_conv3d_pair_wfrag_bytes(c) for c in (8, 16, 32)] == [9 * 2048, 18 * 2048, 36 * 2048]
    assert L.svs_conv3d_rows_wfrag_bytes(16) == 14 * 2048 and L.svs_conv3d_s2c8_wfrag_bytes() == 9 * 2048
    assert L.svs_conv2d_mfma_wfrag_bytes(16, 20, 5) == 2 * 13 * 2048 and L.svs_deconv2d_mfma_wfrag_bytes(32, 16) == 9 * 2048
    assert L.svs_conv3d_gemm_wfrag_bytes(64, 64, 0) == 54 * 4 * 2048 and L.svs_conv3d_gemm_wfrag_bytes(16, 8, 1) == 4 * 4 * 2048
    assert L.svs_version() == 101
