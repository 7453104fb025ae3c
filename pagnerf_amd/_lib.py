"""ctypes binding of libpagnerf_hip.so, derived at import from include/pagnerf_hip.h: parse_header() reads the header's constants, argument structs
and prototypes, so the header is the only record of the C ABI.

The product path has NO CPU fallback: if the library is missing or a GPU tensor is not handed
in, calls raise.  Import of this module alone never touches the GPU.
"""
import ctypes
import os
import re

import torch

from . import build as _build

_C_TYPES = {"void": None, "char": ctypes.c_char, "unsigned char": ctypes.c_ubyte, "uint8_t": ctypes.c_uint8, "uint16_t": ctypes.c_uint16,
            "int": ctypes.c_int, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64,
            "float": ctypes.c_float, "double": ctypes.c_double}
_DECLARATOR = re.compile(r"(\w+(?: \w+)*?) ?((?:\* ?)*)(\w+) ?((?:\[\w+\])*)")      # the type's words, the stars, the name, the array extents


def _int(expr, consts):
    """The header's integer constant expressions: a literal or `literal << literal`, in parentheses and behind an (int64_t) cast or not, or a constant's name."""
    e = re.sub(r"\(\s*int64_t\s*\)|[()\s]", "", expr)
    m = re.fullmatch(r"(-?\d+)(?:<<(\d+))?", e)
    if m:
        return int(m.group(1)) << int(m.group(2) or 0)
    if e not in consts:
        raise ValueError("pagnerf_hip.h: cannot evaluate %r" % expr)
    return consts[e]


def _declare(text, types, consts, returns=False):
    """One C declaration, `const float *a, *b[3]` -> [(name, ctype), ...].  A pointer to a pag_* struct is POINTER(that struct), a returned `char *` a
    c_char_p, every other pointer a c_void_p."""
    out, base = [], ""
    for d in " ".join(re.sub(r"\b(const|struct)\b", " ", text).split()).split(","):
        m = _DECLARATOR.fullmatch((base + " " + d.strip()).strip())
        if not m:
            raise ValueError("pagnerf_hip.h: cannot split the declarator %r of %r" % (d, text))
        base, stars, name, extents = m.groups()
        if base not in types:
            raise ValueError("pagnerf_hip.h: unknown type %r in %r" % (base, text))
        t = types[base]
        if "*" in stars:
            t = ctypes.POINTER(t) if base.startswith("pag_") and stars.count("*") == 1 else ctypes.c_char_p if returns and base == "char" else ctypes.c_void_p
        elif t is None:
            raise ValueError("pagnerf_hip.h: %r declares a void value" % text)
        for n in reversed(re.findall(r"\w+", extents)):
            t = t * _int(n, consts)
        out.append((name, t))
    return out


def parse_header(text):
    """(constants, structs, prototypes) of a header written as include/pagnerf_hip.h is: {"PAG_X": int} from the defines and the enums,
    {"pag_x": ctypes.Structure class}, and {"pag_f": (restype, [argtypes])}.  Anything it does not recognise raises: it never skips."""
    code = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts, lines = {}, []
    for line in re.sub(r"^#ifdef __cplusplus$.*?^#endif$", "", code, flags=re.S | re.M).splitlines():     # the extern "C" brackets
        line = line.strip()
        m = re.fullmatch(r"#define (PAG_\w+) +(\S.*)", line)
        if m:
            consts[m.group(1)] = _int(m.group(2), consts)
        elif not line.startswith("#"):
            lines.append(line)
        elif not re.fullmatch(r"#(ifndef \w+_H|define \w+_H|include <stdint\.h>|endif)", line):       # the include guard
            raise ValueError("pagnerf_hip.h: unknown preprocessor line %r" % line)
    body, statements, depth, start = "\n".join(lines), [], 0, 0
    for i, ch in enumerate(body):
        depth += (ch == "{") - (ch == "}")
        if ch == ";" and depth == 0:
            statements.append(" ".join(body[start:i].split()))
            start = i + 1
    if body[start:].strip():
        raise ValueError("pagnerf_hip.h: no ';' after %r" % body[start:].strip()[:80])
    bodies, rest = {}, []
    for s in statements:                                                        # the constants and every struct's class first ...
        enum, struct = re.fullmatch(r"enum ?\{(.*)\}", s), re.fullmatch(r"typedef struct (pag_\w+) ?\{(.*)\} ?(\w+)", s)
        if enum:
            value = -1
            for item in enum.group(1).split(","):
                name, _, expr = (w.strip() for w in item.partition("="))
                if not re.fullmatch(r"PAG_\w+", name):
                    raise ValueError("pagnerf_hip.h: cannot read the enumerator %r" % item)
                value = consts[name] = _int(expr, consts) if expr else value + 1
        elif struct and struct.group(1) == struct.group(3):
            bodies[struct.group(1)] = struct.group(2)
        else:
            rest.append(s)
    structs = {name: type(name, (ctypes.Structure,), {"__doc__": "%s (include/pagnerf_hip.h)." % name}) for name in bodies}
    types = dict(_C_TYPES, **structs)
    for name, fields in bodies.items():                                         # ... then the fields, which may point to any of them
        *fields, last = fields.split(";")
        if last.strip():
            raise ValueError("pagnerf_hip.h: no ';' after %r in %s" % (last.strip(), name))
        structs[name]._fields_ = [f for decl in fields for f in _declare(decl, types, consts)]
    sigs = {}
    for s in rest:
        m = re.fullmatch(r"(.*?\W)(pag_\w+) ?\((.*)\)", s)
        if m:
            params = [] if m.group(3).strip() == "void" else [_declare(p, types, consts) for p in m.group(3).split(",")]
            if any(issubclass(t, ctypes.Array) for (_, t), in params):
                raise ValueError("pagnerf_hip.h: array parameter in %r" % s)
            sigs[m.group(2)] = (_declare(m.group(1) + m.group(2), types, consts, returns=True)[0][1], [t for (_, t), in params])
        elif not (re.fullmatch(r"struct (pag_\w+)", s) and s.split()[1] in structs):                     # a forward declaration
            raise ValueError("pagnerf_hip.h: cannot read %r" % s[:120])
    missed = set(re.findall(r"\b(pag_\w+)\s*\(", code)) - set(sigs)
    if missed:
        raise ValueError("pagnerf_hip.h: no prototype read for %s" % sorted(missed))
    return consts, structs, sigs


with open(_build.HEADER) as _fh:
    _CONSTS, _STRUCTS, _SIGS = parse_header(_fh.read())
globals().update({name[len("PAG_"):]: value for name, value in _CONSTS.items()})            # F32, ACT_SOFTMAX, LAYOUT_XCD8, ABI_VERSION, VIS_MAX_ID, ...
MlpFwdArgs = _STRUCTS["pag_mlp_fwd_args"]
HeadCompositeArgs = _STRUCTS["pag_head_composite_args"]
MlpBwdArgs = _STRUCTS["pag_mlp_bwd_args"]
WgradLayer = _STRUCTS["pag_wgrad_layer"]
DeepMlpArgs = _STRUCTS["pag_deep_mlp_args"]
Mlp128FwdArgs = _STRUCTS["pag_mlp128_fwd_args"]
Mlp128BwdArgs = _STRUCTS["pag_mlp128_bwd_args"]
VmArgs = _STRUCTS["pag_vm_args"]
SampleMode = _STRUCTS["pag_sample_mode"]
LabelPlane = _STRUCTS["pag_label_plane"]
CocoTables = _STRUCTS["pag_coco_tables"]
Bup20PrepareArgs = _STRUCTS["pag_bup20_prepare_args"]
VisArgs = _STRUCTS["pag_vis_args"]

_DT = {torch.float32: F32, torch.float16: F16, torch.bfloat16: BF16}
MLP128_BATCH, MLP128_MAX_GRID = 256, 256      # samples per workgroup batch, workgroups per launch (the forward / backward grid-stride beyond their product)

EXPORTS = tuple(_SIGS)
_lib = None


def load():
    """dlopen the C-ABI library (building is __graft_entry__.build()'s job); raises if absent."""
    global _lib
    if _lib is None:
        path = _build.LIB
        if not os.path.exists(path):
            raise RuntimeError("libpagnerf_hip.so not found at %s - run `python -m pagnerf_amd.build` "
                               "(there is no CPU fallback for the HIP path)" % path)
        lib = ctypes.CDLL(path)
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.pag_abi_version() != ABI_VERSION:
            raise RuntimeError("libpagnerf_hip.so ABI version mismatch")
        _lib = lib
    return _lib


def check(rc, name):
    if rc != 0:
        msg = load().pag_last_error_string().decode("utf-8", "replace")
        raise RuntimeError("%s failed (%d): %s" % (name, rc, msg))


def dtype_code(t):
    return _DT[t.dtype]


def ptr(t):
    """Device pointer of a contiguous GPU tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("pagnerf_amd: expected a GPU tensor (the HIP path has no CPU fallback), got %s" % t.device)
    if not t.is_contiguous():
        raise RuntimeError("pagnerf_amd: tensor must be contiguous")
    return t.data_ptr()


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream():
    """The raw handle of torch's current stream on the current device.  torch.cuda.current_stream() builds a Stream object per call (~10 us: a tenth of
    the host time of a forward-only trace, which asks nine times); the C-level getter returns the same handle in well under a microsecond."""
    if _RAW_STREAM is not None:
        return _RAW_STREAM(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def host_floats(values):
    """python/numpy/torch-CPU float sequence -> ctypes float array (kept alive by the caller)."""
    if values is None:
        return None
    if isinstance(values, torch.Tensor):
        values = values.detach().cpu().float().reshape(-1).tolist()
    else:
        import numpy as np
        values = np.asarray(values, dtype=np.float32).reshape(-1).tolist()
    return (ctypes.c_float * len(values))(*values)
