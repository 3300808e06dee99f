"""ctypes binding of the C ABI in include/homan_amd.h (libhoman_amd.so).

The product path has no CPU fallback: if the HIP library is missing or a call fails, this
module raises.  Device pointers come from torch tensors (plumbing only: memory + streams).
"""
import ctypes
import os
import re

import torch

from . import build as _build

_LIB = None
_VP, _I, _F, _SZ, _L = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_long
# The closed type tables of the header: what is passed by value, and what a pointer (always a c_void_p here) may point to.
_BY_VALUE = {"int": _I, "float": _F, "long": _L, "size_t": _SZ, "hipStream_t": _VP}
_POINTEES = {"void", "float", "double", "int", "unsigned char", "HmSilRender"}


class HomanAmdError(RuntimeError):
    pass


def _ctype(decl, named=True):
    """'const float* const* g_terms' -> (c_void_p, 'g_terms'); 'size_t' with named=False (a return type) -> (c_size_t, None).
    A type outside the two tables raises: nothing defaults to int."""
    words = decl.replace("*", " * ").split()
    name = words.pop() if named and words else None
    base = " ".join(w for w in words if w not in ("*", "const"))
    if (named and not (name or "").isidentifier()) or base not in (_POINTEES if "*" in words else _BY_VALUE):
        raise HomanAmdError(f"include/homan_amd.h: no ctypes mapping for `{decl.strip()}`")
    return (_VP if "*" in words else _BY_VALUE[base]), name


def parse_header(text):
    """The ABI as include/homan_amd.h spells it -> ({name: (restype, argtypes)}, [(field of HmSilRender, ctype)]).
    Strict: once comments, preprocessor lines and the extern "C" braces are gone, every statement must be the hipStream_t
    typedef, the HmSilRender struct or an hm_* prototype over the types of _ctype; anything else raises HomanAmdError."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = re.sub(r'extern "C" \{(.*)\}', r"\1", text, flags=re.S)
    sigs, fields = {}, []

    def take_struct(m):
        for decl in filter(str.strip, m.group(1).split(";")):
            first, *more = decl.split(",")                   # `int B, V, F`: by-value members only
            ctype, name = _ctype(first)
            names = [name] + [n.strip() for n in more]
            if more and (ctype is _VP or not all(n.isidentifier() for n in names)):
                raise HomanAmdError(f"include/homan_amd.h: member list `{decl.strip()}` not understood")
            fields.extend((n, ctype) for n in names)
        return ""
    text = re.sub(r"typedef struct HmSilRender \{(.*?)\} HmSilRender;", take_struct, text, flags=re.S)
    for stmt in filter(str.strip, text.split(";")):
        if stmt.split() == ["typedef", "struct", "ihipStream_t*", "hipStream_t"]:
            continue
        m = re.fullmatch(r"\s*(.+?)\b(hm_\w+)\s*\((.*)\)\s*", stmt, flags=re.S)
        if not m or m.group(2) in sigs:
            raise HomanAmdError(f"include/homan_amd.h: statement `{stmt.strip()}` not understood")
        params = m.group(3).strip()
        sigs[m.group(2)] = (_ctype(m.group(1), named=False)[0],
                            [] if params == "void" else [_ctype(p)[0] for p in params.split(",")])
    return sigs, fields


class SilRender(ctypes.Structure):
    """HmSilRender of include/homan_amd.h: one render of hm_sil_fwd_multi (fields as the arguments of hm_sil_fwd_clips)"""


# name -> (restype, argtypes), and the struct's members: read off the header, the one place that spells the ABI
with open(_build.HEADER) as _fh:
    _SIGNATURES, SilRender._fields_ = parse_header(_fh.read())


def sil_renders(renders):
    """[dict of HmSilRender fields (tensors or ints / floats; missing = NULL / 0)] -> ctypes array for hm_sil_fwd_multi.
    The array is read by the library when the call is made (or captured); the tensors must outlive the launches."""
    arr = (SilRender * len(renders))()
    for r, d in zip(arr, renders):
        for k, v in d.items():
            setattr(r, k, ptr(v) if isinstance(v, torch.Tensor) else v)
    assert ctypes.sizeof(SilRender) == lib().hm_sil_render_bytes(), "HmSilRender layout differs from the library's"
    return arr


def lib():
    """Load libhoman_amd.so (after torch, so the HIP runtime already in the process is reused)."""
    global _LIB
    if _LIB is None:
        path = os.environ.get("HOMAN_AMD_LIB", _build.LIB_PATH)      # (A/B runs of kernel variants: tools/ab_build.sh)
        if not os.path.exists(path):
            raise HomanAmdError(
                f"{path} not found: build it with `python -m homan_amd.build` (hipcc, gfx950). "
                "homan_amd has no CPU fallback.")
        _LIB = ctypes.CDLL(path)
        for name, (res, args) in _SIGNATURES.items():
            try:
                fn = getattr(_LIB, name)
            except AttributeError as exc:
                raise HomanAmdError(f"{path} does not export {name}; rebuild it") from exc
            fn.restype, fn.argtypes = res, args
    return _LIB


def exported_symbols():
    return sorted(_SIGNATURES)


def ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "homan_amd ops need contiguous device tensors"
    return t.data_ptr()


def aligned(t, nbytes):
    """`t` itself when its address is a multiple of `nbytes`, else an equal copy in an allocation of its own (torch's allocators
    hand out far more than 16 bytes of alignment).  For caller-supplied tensors that go to a parameter whose alignment
    requirement exceeds the element size (include/homan_amd.h, Conventions): a contiguous view such as `x.view(-1)[1:1 + n]` is
    only element-aligned.  Buffers this package allocates itself need nothing."""
    if t is None or t.data_ptr() % nbytes == 0:
        return t
    return t.clone(memory_format=torch.contiguous_format)


def stream():
    return torch.cuda.current_stream().cuda_stream


def terms(pairs):
    """[(tensor or None, weight), ...] -> (host array of device pointers, host array of floats, n) for the entry points
    that take a weighted list of per-vertex gradients (read by the library at launch time)."""
    live = [(t, w) for t, w in pairs if t is not None]
    n = len(live)
    ptrs = (ctypes.c_void_p * max(n, 1))(*[ptr(t) for t, _ in live])
    ws = (ctypes.c_float * max(n, 1))(*[float(w) for _, w in live])
    return ptrs, ws, n


def check(rc, what):
    if rc != 0:
        raise HomanAmdError(f"{what} failed with code {rc}")


# Graphs are kept alive for the life of the process.  ROCm 7.0's graph executor has
# crashed in hip::Graph::UpdateStreams at the first replay of a NEW graph after several dozen graphs had been created AND
# destroyed in the process - a test suite, or a fitting process that walks a dataset clip by clip, one stepper per clip.
# Graphs that are never destroyed do not trigger it, and a captured graph here owns no large buffer (the steppers allocate
# before capture): a few kilobytes per fitted clip.
_KEPT_GRAPHS = []


def new_graph():
    g = torch.cuda.CUDAGraph()
    _KEPT_GRAPHS.append(g)
    return g


# ... which holds for the FUSED steppers only.  A graph that captures HOMan.forward + autograd (jointopt.GraphStepper, the
# eager-style loop of pose_optimization._graph_loop) owns every activation of the iteration in its private memory pool -
# hundreds of MB per clip / frame - and keeping such graphs alive kept that memory too.  Those captures share ONE pool
# (`torch.cuda.graph(g, pool=autograd_pool())`): the activations are temporaries, freed by the end of the capture, so the next
# capture reuses the same blocks - the graphs stay alive (no destroy, no crash), the memory is bounded by the largest
# iteration plus the few small tensors each capture keeps (tools/soak_dataset.py walks a dataset in graph mode).  Sound
# because steppers are replayed one at a time and nothing but their kept outputs lives across replays.
_AUTOGRAD_POOL = None


def autograd_pool():
    global _AUTOGRAD_POOL
    if _AUTOGRAD_POOL is None:
        _AUTOGRAD_POOL = torch.cuda.graph_pool_handle()
    return _AUTOGRAD_POOL
