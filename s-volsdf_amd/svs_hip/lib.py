"""ctypes binding of libsvolsdf_hip.so, derived from the C-ABI's one declaration, include/svolsdf_hip.h.

The header is parsed once at import: its prototypes give SIGNATURES, its two job structs the Structure classes, its
#defines and its enum the constants.  Nothing about the ABI is restated here.

The product path has NO CPU fallback: if the library is missing or a call fails, this raises.
"""
import ctypes
import os
import re
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_longlong, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# SVS_LIB_PATH: another build of the same library (A/B timing of kernel variants on one box, tools/ab_variant.sh)
LIB_PATH = os.environ.get("SVS_LIB_PATH") or os.path.join(os.path.dirname(_HERE), "lib", "libsvolsdf_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "svolsdf_hip.h")

_lib = None


class SvsError(RuntimeError):
    pass


# ---- the header's C subset -------------------------------------------------------------------------------------------
# Types passed by value, and what a pointer may point to.  Everything else is refused by name: the parser never guesses.
_SCALARS = {"int": c_int, "float": c_float, "double": c_double, "size_t": c_size_t, "long long": c_longlong}
_POINTEES = set(_SCALARS) | {"void", "char", "unsigned char", "uint8_t", "short", "unsigned int", "unsigned long long"}
_TOKENS = re.compile(r"\w+|\*").findall
_NOT_A_DECLARATOR = re.compile(r"[^\w\s*]").search          # brackets, parentheses, initialisers, bit fields


def _ctype(base, stars, host, pointees):
    """The ctypes type of `base` behind `stars` asterisks (host: the declaration carries SVS_HOST), None if no rule gives one."""
    if stars == 0 and not host:
        return _SCALARS.get(base)
    if base == "char" and stars == 1 and not host:
        return c_char_p
    if base in pointees and stars in (1, 2):
        if not host:
            return c_void_p                  # a device pointer, or an address the call hands on: a plain address
        if stars == 2:
            return POINTER(c_void_p)
        if base in _SCALARS:
            return POINTER(_SCALARS[base])
    return None


def _declarator(text, pointees, what):
    """`const float* const SVS_HOST* name` -> (name, ctype).  The name is the last word; `const` says nothing about the ABI."""
    tokens = _TOKENS(text)
    words = [t for t in tokens if t not in ("*", "const", "SVS_HOST")]
    ctype = None
    if len(words) >= 2 and not _NOT_A_DECLARATOR(text):
        ctype = _ctype(" ".join(words[:-1]), tokens.count("*"), "SVS_HOST" in tokens, pointees)
    if ctype is None:
        raise SvsError(f"{HEADER_PATH}: {what}: cannot classify `{' '.join(text.split())}`")
    return words[-1], ctype


def _struct_fields(name, body):
    """`const float *a0, *b0; long long sa0, sb0;` -> [("a0", c_void_p), ("b0", c_void_p), ("sa0", c_longlong), ...]"""
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        first, *more = decl.split(",")
        fields.append(_declarator(first, _POINTEES, f"struct {name}"))
        base = " ".join(re.findall(r"\w+", first)[:-1])
        for m in more:                       # `, *b0` / `, sb0`: the first declarator's base type, its own asterisk
            if not re.fullmatch(r"\s*\*?\s*\w+\s*", m):
                raise SvsError(f"{HEADER_PATH}: struct {name}: cannot parse field `{decl}`")
            fields.append(_declarator(base + " " + m, _POINTEES, f"struct {name}"))
    return fields


def parse_header(text):
    """The header's text -> (constants, structs, signatures): {name: int}, {struct name: [(field, ctype)]} and
    {function: (restype, [argtypes])}.  Raises SvsError, naming it, for anything that is not one of: a comment, an #include /
    #ifdef / #ifndef / #endif line, a #define of an integer or of nothing, extern "C", an enum of integers, a typedef struct, a prototype."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants, structs, signatures = {}, {}, {}

    def directive(m):
        line = m.group(1).strip()
        d = re.fullmatch(r"define\s+(\w+)(?:\s+\(?\s*(-?\d+)\s*\)?)?", line)
        if d and d.group(2) is not None:
            constants[d.group(1)] = int(d.group(2))
        elif not d and not re.match(r"(include|ifdef|ifndef|endif)\b", line):
            raise SvsError(f"{HEADER_PATH}: cannot parse directive `#{line}`")
        return " "
    text = re.sub(r"^[ \t]*#([^\n]*)$", directive, text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", text, flags=re.S)

    def enum(m):
        for item in filter(None, (i.strip() for i in m.group(1).split(","))):
            e = re.fullmatch(r"(\w+)\s*=\s*(-?\d+)", item)
            if not e:
                raise SvsError(f"{HEADER_PATH}: enum: cannot parse `{item}`")
            constants[e.group(1)] = int(e.group(2))
        return " "
    text = re.sub(r"\benum\s*\{([^}]*)\}\s*;", enum, text)

    def struct(m):
        if m.group(1) != m.group(3):
            raise SvsError(f"{HEADER_PATH}: typedef struct {m.group(1)} is named {m.group(3)}")
        structs[m.group(1)] = _struct_fields(m.group(1), m.group(2))
        return " "
    text = re.sub(r"\btypedef\s+struct\s+(\w+)\s*\{([^}]*)\}\s*(\w+)\s*;", struct, text)

    pointees = _POINTEES | set(structs)
    for decl in filter(None, (d.strip() for d in text.split(";"))):
        m = re.fullmatch(r"([\w\s*]+?)\b(\w+)\s*\(([^()]*)\)", decl)
        if not m:
            raise SvsError(f"{HEADER_PATH}: cannot parse declaration `{' '.join(decl.split())[:80]}`")
        name, params = m.group(2), m.group(3).strip()
        _, restype = _declarator(m.group(1) + " " + name, pointees, f"{name}, return type")
        args = [] if params == "void" else [_declarator(p, pointees, name)[1] for p in params.split(",")]
        signatures[name] = (restype, args)
    return constants, structs, signatures


def _structure(cls_name, fields, c_name):
    return type(cls_name, (ctypes.Structure,), {"_fields_": fields, "__doc__": f"{c_name} of include/svolsdf_hip.h"})


try:
    with open(HEADER_PATH) as _f:
        _CONSTANTS, _STRUCTS, SIGNATURES = parse_header(_f.read())      # SIGNATURES: name -> (restype, argtypes)
    WGradJob = _structure("WGradJob", _STRUCTS["svs_wgrad_job"], "svs_wgrad_job")
    UnpackJob = _structure("UnpackJob", _STRUCTS["svs_unpack_job"], "svs_unpack_job")
    ABI_VERSION = _CONSTANTS["SVS_ABI_VERSION"]     # svs_version() of the library this binding is derived for
    EINVAL, ESHAPE, ENOCONV, EOVERFLOW = (_CONSTANTS["SVS_E" + n] for n in ("INVAL", "SHAPE", "NOCONV", "OVERFLOW"))
    MMA_F32, MMA_F16X2, MMA_F16X2_HALF = (_CONSTANTS["SVS_MMA_" + n] for n in ("F32", "F16X2", "F16X2_HALF"))
    PAINT_BEST, PAINT_ONE_SIDED = (_CONSTANTS["SVS_PAINT_" + n] for n in ("BEST", "ONE_SIDED"))
    ATLAS_CELL_MAJOR = _CONSTANTS["SVS_ATLAS_CELL_MAJOR"]
    MESH_USED, MESH_BOUNDARY, MESH_NONMANIFOLD = (_CONSTANTS["SVS_MESH_" + n] for n in ("USED", "BOUNDARY", "NONMANIFOLD"))
    SMOOTH_FIXED, SMOOTH_CURVE, SMOOTH_FREE = (_CONSTANTS["SVS_SMOOTH_" + n] for n in ("FIXED", "CURVE", "FREE"))
except (OSError, KeyError) as _e:
    raise SvsError(f"{HEADER_PATH}: the binding is derived from this header and cannot do without it: {_e!r}") from _e


def load():
    """Load the shared library once; raises SvsError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  -- first, so that the HIP runtime torch ships is the one this library binds to
    if not os.path.exists(LIB_PATH):
        raise SvsError(f"{LIB_PATH} not found: run `python s-volsdf_amd/build.py` (there is no CPU fallback)")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the header and the library disagree
        fn.restype = res
        fn.argtypes = args
    have = lib.svs_version()
    if have != ABI_VERSION:
        raise SvsError(f"{LIB_PATH} has ABI version {have}, the header this binding reads declares {ABI_VERSION}: "
                       "rebuild with `python s-volsdf_amd/build.py --force`")
    if os.environ.get("SVS_DETERMINISTIC") == "1":
        lib.svs_set_deterministic(1)
    _lib = lib
    return lib


def deterministic():
    """SVS_DETERMINISTIC=1 (or svs_set_deterministic(1)): weight gradients summed in one fixed order, steps on one stream."""
    return bool(load().svs_get_deterministic())


def check(rc, what=""):
    if rc != 0:
        msg = load().svs_last_error_string()
        raise SvsError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")
