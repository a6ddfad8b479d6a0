"""ctypes binding of liborp_hip.so (the C ABI declared in include/orp_hip.h).

The product path has NO CPU fallback: if the HIP library is missing the import of any operator fails loudly.
PyTorch is used for device memory, the current stream and (elsewhere) torch.distributed only.

The header is the only declaration of the ABI: the signatures, the argument structs and the ORP_* constants below are parsed
from it at import (`parse_header`), and a declaration the parser cannot map is an error, never a skipped entry.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ORP_HIP_LIB") or os.path.join(_HERE, "csrc", "liborp_hip.so")   # ORP_HIP_LIB: dev aid (instrumented builds)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "orp_hip.h")


class OrpHipError(RuntimeError):
    pass


_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "uint32_t": ctypes.c_uint32, "float": ctypes.c_float,
            "double": ctypes.c_double, "size_t": ctypes.c_size_t, "long": ctypes.c_long, "long long": ctypes.c_longlong,
            "int64_t": ctypes.c_longlong}
_POINTEES = set(_SCALARS) | {"void", "char", "uint8_t"}


def _ctype(spec, structs, decl, field=False, result=False):
    """ctypes type of the C type `spec` (no declarator) as an argument, a struct field or a function's result.  Pointers are
    c_void_p, except a field that points to a parsed struct and a `char*` result; `decl` is what the error quotes."""
    base = " ".join(w for w in spec.replace("*", " ").split() if w != "const")
    stars = spec.count("*")
    if result and (base, stars) in (("void", 0), ("char", 1)):
        return ctypes.c_char_p if stars else None
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars and not result and (base in _POINTEES or base in structs):
        return ctypes.POINTER(structs[base]) if field and stars == 1 and base in structs else ctypes.c_void_p
    raise OrpHipError("orp_hip.h: cannot map the type `%s` in `%s`" % (spec.strip(), decl))


def _declarator(text, decl):
    """`<type> <name>` or `<type> <name>[<n>]` -> (type, name, n or None)."""
    m = re.fullmatch(r"([\w\s*]*[\s*])(\w+)\s*(?:\[\s*(\d+)\s*\])?", text.strip())
    if not m or m.group(2) in _POINTEES or m.group(2) == "const":     # (an unnamed `long long` is not a `long` called long)
        raise OrpHipError("orp_hip.h: cannot parse `%s` in `%s`" % (text.strip(), decl))
    return m.group(1), m.group(2), m.group(3) and int(m.group(3))


def parse_header(text):
    """C header text -> (signatures {name: (restype, argtypes)}, structs {name: ctypes.Structure}, constants {ORP_*: int})."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    signatures, structs, constants = {}, {}, {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(ORP_\w+)[ \t]+(\S.*?)[ \t]*$", text, flags=re.M):
        m = re.fullmatch(r"\(\s*(-?\s*\w+)\s*\)|(-?\s*\w+)", value)
        try:
            constants[name] = int((m.group(1) or m.group(2)).replace(" ", ""), 0)
        except (AttributeError, ValueError):
            raise OrpHipError("orp_hip.h: `#define %s %s` is not an integer" % (name, value))
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", text, flags=re.S)
    depth, start, decls = 0, 0, []
    for m in re.finditer(r"[{};]", text):       # a declaration ends at a `;` outside braces
        depth += (m.group() == "{") - (m.group() == "}")
        if m.group() == ";" and depth == 0:
            decls.append(" ".join(text[start:m.start()].split()))
            start = m.end()
    if text[start:].strip():
        raise OrpHipError("orp_hip.h: unfinished declaration `%s`" % " ".join(text[start:].split()))
    for decl in decls:
        st = re.fullmatch(r"typedef struct(?: \w+)? ?\{([^{}]*)\} ?(\w+)", decl)
        fn = re.fullmatch(r"([\w\s*]*[\s*])(\w+) ?\(([^()]*)\)", decl)
        if (st and st.group(2) in structs) or (fn and fn.group(2) in signatures):
            raise OrpHipError("orp_hip.h: declared twice: `%s`" % decl)
        if st:
            fields = []
            for line in filter(None, (f.strip() for f in st.group(1).split(";"))):
                first, *more = line.split(",")
                spec = _declarator(first, line)[0]
                if more and "*" in line:        # `float *a, *b` / `float* a, b`: the star binds to one name only
                    raise OrpHipError("orp_hip.h: a pointer in the comma list `%s`" % line)
                for d in [first] + [spec + " " + other for other in more]:
                    _, name, n = _declarator(d, line)
                    t = _ctype(spec, structs, line, field=True)
                    fields.append((name, t if n is None else t * n))
            structs[st.group(2)] = type(st.group(2), (ctypes.Structure,), {"_fields_": fields})
        elif fn:
            args = []
            for p in ([] if fn.group(3).strip() == "void" else fn.group(3).split(",")):
                spec, _, n = _declarator(p, decl)
                if n is not None:
                    raise OrpHipError("orp_hip.h: an array argument `%s` in `%s`" % (p.strip(), decl))
                args.append(_ctype(spec, structs, decl))
            signatures[fn.group(2)] = (_ctype(fn.group(1), structs, decl, result=True), args)
        else:
            raise OrpHipError("orp_hip.h: cannot parse the declaration `%s`" % decl)
    return signatures, structs, constants


def _load_header():
    if not os.path.exists(HEADER_PATH):
        raise OrpHipError("orientedreppoints_amd: the C header %s is missing; the binding is derived from it" % HEADER_PATH)
    with open(HEADER_PATH) as f:
        return parse_header(f.read())


# name -> (restype, argtypes); name -> ctypes.Structure; ORP_* -> int: include/orp_hip.h, parsed once per process
_SIGNATURES, _STRUCTS, _CONSTANTS = _load_header()
ORP_OK, ORP_EINVAL, ORP_EWORKSPACE, ORP_ETOOBIG = (_CONSTANTS[k] for k in ("ORP_OK", "ORP_EINVAL", "ORP_EWORKSPACE", "ORP_ETOOBIG"))
ORP_NMS_MAX_BOXES = _CONSTANTS["ORP_NMS_MAX_BOXES"]


def struct(name):
    """The ctypes.Structure of the header's `typedef struct { ... } name;` (field names and order as declared)."""
    return _STRUCTS[name]


_lib = None


def lib():
    """Load liborp_hip.so (once).  Raises if it has not been built: there is deliberately no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OrpHipError(
                "orientedreppoints_amd: HIP library %s is missing. Build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950). "
                "There is no CPU fallback for the hot path." % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)          # AttributeError = the .so is stale vs the header: also loud
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc, what):
    if rc != ORP_OK:
        names = {ORP_EINVAL: "ORP_EINVAL", ORP_EWORKSPACE: "ORP_EWORKSPACE", ORP_ETOOBIG: "ORP_ETOOBIG"}
        raise OrpHipError("%s failed: %s" % (what, names.get(rc, "hipError %d" % rc)))


def call(name, device, *args):
    """one launch: the library's entry point `name`, looked up at call time, under the device guard, its return code checked"""
    with torch.cuda.device(device):
        rc = getattr(lib(), name)(*args)
    check(rc, name)


def tile_query(name, n, *shape):
    """the n integers the library's `name`(shape..., n int pointers) fills for a launch of this shape, or None where it returns 0"""
    v = [ctypes.c_int() for _ in range(n)]
    if not getattr(lib(), name)(*[int(s) for s in shape], *[ctypes.byref(t) for t in v]):
        return None
    return tuple(t.value for t in v)


def ptr(t):
    """Device (or host) address of a contiguous tensor, or NULL."""
    if t is None:
        return None
    assert t.is_contiguous(), "orientedreppoints_amd: tensor must be contiguous"
    return ctypes.c_void_p(t.data_ptr())


def stream_of(t):
    """hipStream_t of PyTorch's current stream on the tensor's device (ops are stream-ordered, never blocking)."""
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def require_cuda(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError("%s must be a CUDA tensor" % name)


_workspaces = {}
_keepalive = None          # list while a GraphedInference capture collects the cached tensors its graph reads


def workspace(device, nbytes):
    """Scratch bytes for ONE op call on PyTorch's current stream of `device`.

    * eager: a cached, growing buffer per (device, stream).  A buffer is only ever used by work queued on the stream it
      is keyed by, so replacing it on growth hands the old block back to the caching allocator in stream order (no
      cross-stream reuse race, no record_stream needed).
    * during a stream capture: a fresh allocation from the capturing graph's private memory pool -- the graph owns its
      scratch for as long as it lives, and nothing an eager call does later (a 20 k-box merge NMS growing the cached
      buffer, a training step, the capacity-overflow fallback) can free or move memory a replay writes to.
    """
    nbytes = max(int(nbytes), 1)
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(nbytes, dtype=torch.uint8, device=device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    key = (idx, torch.cuda.current_stream(device).cuda_stream)
    w = _workspaces.get(key)
    if w is None or w.numel() < nbytes:
        if key not in _workspaces and len(_workspaces) >= 32:   # short-lived side streams: drop the oldest buffer only
            _workspaces.pop(next(iter(_workspaces)))           # (its block goes back to the allocator in stream order)
        w = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _workspaces[key] = w
    return w


def keep_for_graph(t):
    """Cached tensors (packed DeformConv weights, folded BatchNorm affines) a captured graph reads must outlive their
    cache entry: while a GraphedInference capture is collecting, remember them on the graph's owner."""
    if _keepalive is not None and t is not None:
        _keepalive.append(t)
    return t
