"""ctypes binding of libx2g.so, read from the C ABI's one declaration, include/x2g.h.

``parse_header`` turns the header's text into the argument and return types of every function, a
``ctypes.Structure`` per ``typedef struct`` and the integer ``#define``s; nothing of the ABI is restated in
Python.  It reads the subset of C the header is written in and raises on anything else.

The library is loaded after ``torch`` so that it binds to the HIP runtime PyTorch already
loaded (same soname), and every call is enqueued on PyTorch's current stream.  There is no
fallback: if the library or a GPU is missing, the product path raises.
"""
from __future__ import annotations

import ctypes
import keyword
import os
import re

import torch  # noqa: F401  (must be imported before the HIP library is loaded)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("X2G_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libx2g.so"))
HEADER_PATH = os.environ.get("X2G_HEADER",
                             os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "x2g.h"))
# the staged entry points' header, next to x2g.h: compiled into the same library, outside the recorded ABI
STAGED_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "x2g_staged.h")
# the multi-target entry points' header (the K-target readout heads, per-target metrics): a table of its own too
MULTI_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "x2g_multi.h")
# the conv combine pass' header (SBFTransformerConv's concat=False / beta=True): again a table of its own
CONV_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "x2g_conv.h")
# the atom-context chain's header (SBFTransformerV2's per-layer edge term): a table of its own as well
ATOMCTX_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "x2g_atomctx.h")
# the guarded parameter update's header (FlatAdam(skip_nonfinite=True)): one more table of its own
TRAIN_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "x2g_train.h")
# the AO edge features' header (x2gnn.features: the model's input from S and H_core): a table of its own, like the rest
FEATURES_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "x2g_features.h")
# the radius graph's header (x2gnn.graph: bonds and per-molecule counts from positions): a table of its own too
GRAPH_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "x2g_graph.h")
# the one-electron integrals' header (x2gnn.integrals: S and H_core from geometry and a basis set): one more table
INTEGRALS_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "x2g_integrals.h")

_SCALARS = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int": ctypes.c_int,
            "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t}


class _Consts(dict):
    """``#define`` name (without ``X2G_``) -> int.  A macro whose value is no integer literal is kept aside
    and raises when it is asked for."""

    def __init__(self):
        super().__init__()
        self.other = {}

    def __missing__(self, name):
        if name in self.other:
            raise ValueError(f"#define {name} is not an integer literal: {self.other[name]!r}")
        raise KeyError(name)


def _ctype(spec, decl, known, ret=False):
    """The ctypes type of the C type ``spec`` (``decl``: the declaration it stands in, for the message)."""
    words = [w for w in re.findall(r"\w+|\*", spec) if w != "const"]
    base, stars = words[:1], words[1:]
    if len(base) == 1 and all(s == "*" for s in stars):
        if not stars and base[0] in _SCALARS:
            return _SCALARS[base[0]]
        if stars and (base[0] in _SCALARS or base[0] in known or base[0] in ("void", "char")):
            return ctypes.c_char_p if ret and base[0] == "char" and len(stars) == 1 else ctypes.c_void_p
    raise ValueError(f"x2g.h: unknown type {spec.strip()!r} in: {decl}")


def _split(item, decl):
    """(type, name) of a parameter or field ``item``; arrays, bit-fields and function pointers do not match."""
    m = re.fullmatch(r"([\w\s*]+?)\s*\b(\w+)", item.strip())
    if not m:
        raise ValueError(f"x2g.h: cannot read {item.strip()!r} in: {decl}")
    return m[1], m[2]


def parse_header(text, known=()):
    """(SIGNATURES, RESTYPES, STRUCTS, CONSTS) of a header written like include/x2g.h: comments, integer
    ``#define``s, ``typedef struct { scalar or pointer fields } name;`` and function declarations.  Anything
    else raises ValueError quoting the declaration.  ``known``: struct names another header declared, which
    this one may point to."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#[ \t]*ifdef[ \t]+__cplusplus\b.*?^[ \t]*#[ \t]*endif\b[^\n]*", "", text, flags=re.S | re.M)
    consts = _Consts()
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)(.*)$", text, flags=re.M):
        name = name[4:] if name.startswith("X2G_") else name
        try:
            consts[name] = int(value.strip(), 0)
        except ValueError:
            consts.other[name] = value.strip()
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)

    structs = {}

    def struct(m):
        decl = " ".join(m[0].split())
        fields = []
        for item in filter(str.strip, m[1].split(";")):
            spec, name = _split(item, decl)
            fields.append((name + "_" if keyword.iskeyword(name) else name, _ctype(spec, decl, structs)))
        structs[m[2]] = type(m[2], (ctypes.Structure,), {"_fields_": fields, "__doc__": f"{m[2]} (include/x2g.h)."})
        return ""

    text = re.sub(r"\btypedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)

    signatures, restypes = {}, {}
    for decl in filter(None, (" ".join(d.split()) for d in text.split(";"))):
        m = re.fullmatch(r"([\w\s*]+?)\s*\b(\w+)\s*\(([^()]*)\)", decl)
        if not m:
            raise ValueError(f"x2g.h: cannot read the declaration: {decl}")
        args = [] if m[3].strip() == "void" else m[3].split(",")
        signatures[m[2]] = [_ctype(_split(a, decl)[0], decl, (*structs, *known)) for a in args]
        restypes[m[2]] = _ctype(m[1], decl, (*structs, *known), ret=True)
    return signatures, restypes, structs, consts


def _read_header():
    if not os.path.exists(HEADER_PATH):
        raise RuntimeError(f"x2g.h not found at {HEADER_PATH}: set X2G_HEADER to the header libx2g.so was built from")
    with open(HEADER_PATH) as f:
        return f.read()


def _read_functions(path, known=()):
    """(signatures, restypes) of a header next to x2g.h, read like it; it declares functions only (no struct,
    no constant: anything else raises; ``known``: x2g.h's structs it may point to).  Empty when the header is
    absent (an X2G_HEADER of an earlier tree)."""
    if not os.path.exists(path):
        return {}, {}
    with open(path) as f:
        sig, res, structs, consts = parse_header(f.read(), known)
    if structs or consts:
        raise ValueError(f"{os.path.basename(path)} declares more than functions: "
                         f"{sorted(structs) + sorted(consts)}")
    return sig, res


# name -> argtypes / restype of every function, name -> Structure of every typedef struct, and the #defines
SIGNATURES, RESTYPES, STRUCTS, CONSTS = parse_header(_read_header())
# the same for the staged entry points (x2g_staged.h), kept apart: SIGNATURES stays exactly x2g.h's
STAGED_SIGNATURES, STAGED_RESTYPES = _read_functions(STAGED_HEADER_PATH)
# and for the multi-target entry points (x2g_multi.h)
MULTI_SIGNATURES, MULTI_RESTYPES = _read_functions(MULTI_HEADER_PATH)
# and for the conv combine pass (x2g_conv.h; its deferred backward fills an x2g_slab_job of x2g.h)
CONV_SIGNATURES, CONV_RESTYPES = _read_functions(CONV_HEADER_PATH, known=tuple(STRUCTS))
# and for the atom-context chain (x2g_atomctx.h)
ATOMCTX_SIGNATURES, ATOMCTX_RESTYPES = _read_functions(ATOMCTX_HEADER_PATH)
# and for the guarded parameter update (x2g_train.h)
TRAIN_SIGNATURES, TRAIN_RESTYPES = _read_functions(TRAIN_HEADER_PATH)
# and for the AO edge features (x2g_features.h)
FEATURES_SIGNATURES, FEATURES_RESTYPES = _read_functions(FEATURES_HEADER_PATH)
# and for the radius graph (x2g_graph.h)
GRAPH_SIGNATURES, GRAPH_RESTYPES = _read_functions(GRAPH_HEADER_PATH)
# and for the one-electron integrals (x2g_integrals.h)
INTEGRALS_SIGNATURES, INTEGRALS_RESTYPES = _read_functions(INTEGRALS_HEADER_PATH)

_lib = None


def load():
    """Load libx2g.so and declare every entry point (raises if the library is missing)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"libx2g.so not found at {LIB_PATH}: build it (make -C x2-gnn_amd) first")
        lib = ctypes.CDLL(LIB_PATH)
        for name, args in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.argtypes = args
            fn.restype = RESTYPES[name]
        for sigs, res in ((STAGED_SIGNATURES, STAGED_RESTYPES), (MULTI_SIGNATURES, MULTI_RESTYPES),
                          (CONV_SIGNATURES, CONV_RESTYPES), (ATOMCTX_SIGNATURES, ATOMCTX_RESTYPES),
                          (TRAIN_SIGNATURES, TRAIN_RESTYPES), (FEATURES_SIGNATURES, FEATURES_RESTYPES),
                          (GRAPH_SIGNATURES, GRAPH_RESTYPES), (INTEGRALS_SIGNATURES, INTEGRALS_RESTYPES)):
            for name, args in sigs.items():
                # (a library built from an earlier tree, X2G_LIB, has none of them: calling one then raises)
                fn = getattr(lib, name, None)
                if fn is not None:
                    fn.argtypes = args
                    fn.restype = res[name]
        _lib = lib
    return _lib


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


def stream_ptr(device=None):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def check(rc: int, name: str):
    if rc != 0:
        msg = load().x2g_status_string(rc).decode()
        raise RuntimeError(f"{name} failed with status {rc}: {msg}")


def call(name: str, *args):
    check(getattr(load(), name)(*args), name)
