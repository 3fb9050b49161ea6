"""One call path for a kernel and its host twin.

A host twin (`cp_X_host_T` beside `cp_X_T` in include/casapose_hip.h; `_lib.TWINS` finds the pairs, `_lib.TWIN_VARIANTS` their weighted variants, `_lib.TWIN_OUTPUT_VARIANTS` a kernel's geometry with another output, `_lib.TWIN_STEPS` the steps on another kernel's output, `_lib.TWIN_READERS` the readers of one; `_lib.host_twin` reads all five) runs a kernel's arithmetic serially on
host pointers and takes the kernel's arguments minus the trailing stream.  A wrapper therefore writes its argument list once and hands it to
`call`; only where the arrays live differs: `array` converts an input and `alloc` makes a set of outputs, on a device or as NumPy arrays.

`call` refuses, before the library is entered, what the header's pointee types can tell apart: a host pointer for a device entry point (a
GPU fault otherwise), a device pointer for a twin, a wrong element type, a non-contiguous array."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib

# C pointee type of the header -> dtype name, which torch and NumPy share; void* takes any
_DTYPES = {"float": "float32", "double": "float64", "int": "int32", "int32_t": "int32", "uint32_t": "uint32", "uint16_t": "uint16", "uint8_t": "uint8",
           "long long": "int64", "int64_t": "int64"}


def array(a, dtype, device=None):
    """`a` (array, tensor or nested list) as a contiguous `dtype` array: a tensor on `device`, or a NumPy array when device is None"""
    if device is None:
        if hasattr(a, "detach"):
            a = a.detach().cpu().numpy()
        return np.ascontiguousarray(a, dtype=dtype)
    if not hasattr(a, "detach"):
        a = torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
    return a.to(device=device, dtype=getattr(torch, np.dtype(dtype).name)).contiguous()


def alloc(spec: Dict[str, Tuple[tuple, object]], device=None, zero: bool = False) -> dict:
    """{name: (shape, dtype)} -> {name: array}, uninitialised or zeroed: tensors on `device`, or NumPy arrays when device is None"""
    if device is None:
        return {k: (np.zeros if zero else np.empty)(shape, dtype) for k, (shape, dtype) in spec.items()}
    make = torch.zeros if zero else torch.empty
    return {k: make(shape, dtype=getattr(torch, np.dtype(dtype).name), device=device) for k, (shape, dtype) in spec.items()}


def _refusal(a, pointee: str, host: bool, device) -> Optional[str]:
    """why `a` may not be passed for a `pointee*` parameter, or None; device: where the earlier tensors of the call live"""
    tensor = isinstance(a, torch.Tensor)
    if not tensor and not isinstance(a, np.ndarray):
        return "a tensor, a NumPy array or None is expected (got %s)" % type(a).__name__
    cuda, dtype = tensor and a.is_cuda, str(a.dtype).split(".")[-1]
    if host == cuda:
        return "a CUDA tensor for a host twin" if host else "a %s for a device entry point" % ("CPU tensor" if tensor else "NumPy array")
    if cuda and device not in (None, a.device):
        return "a tensor on %s, earlier ones on %s" % (a.device, device)
    if not (a.is_contiguous() if tensor else a.flags.c_contiguous):
        return "the array is not contiguous"
    if pointee != "void" and dtype != _DTYPES.get(pointee):
        return "the array holds %s" % dtype
    return None


def call(name: str, *args, host: bool = False, stream: Optional[int] = None) -> None:
    """The device entry point `name` on `stream` over CUDA tensors, or with host=True its twin over NumPy arrays / CPU tensors.  `args` are the
    device entry's arguments without the stream: scalars pass through, None is a null pointer.  A failing call raises with the name of the
    symbol that was called."""
    lib = _lib.load()
    if _lib.POINTEES.get(name, ())[-1:] != ("void",):
        raise _lib.CasaposeHipError("%s is no entry point of %s that ends in a stream" % (name, _lib.HEADER_PATH))
    if host and _lib.host_twin(name) is None:
        raise _lib.CasaposeHipError("%s has no host twin" % name)
    symbol = _lib.host_twin(name) if host else name
    if host != (stream is None):
        raise _lib.CasaposeHipError("%s: %s" % (symbol, "a host twin takes no stream" if host else "a device call needs a stream"))
    pointees = _lib.POINTEES[name][:-1]
    if len(args) != len(pointees):
        raise _lib.CasaposeHipError("%s takes %d arguments before the stream (got %d)" % (name, len(pointees), len(args)))
    passed, device = [], None
    for i, (a, pointee) in enumerate(zip(args, pointees)):
        if pointee is not None and a is not None:
            why = _refusal(a, pointee, host, device)
            if why:
                raise _lib.CasaposeHipError("%s, argument %d (%s*): %s" % (symbol, i, pointee, why))
            device = None if host else a.device
            a = a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data
        passed.append(a)
    _lib.check(getattr(lib, symbol)(*passed, *(() if host else (stream,))), symbol)
