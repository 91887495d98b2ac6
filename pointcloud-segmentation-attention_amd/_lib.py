"""ctypes binding of libpn2hip.so — the C ABI declared in include/pn2hip.h and pn2plan.h.
Signatures, PN2_* constants and structs are derived from those headers at import (_header.py).

The product path is the HIP library: if it is missing, every op raises; there is no CPU
fallback. `torch` is imported first on purpose: torch ships its own libamdhip64.so (SONAME
libamdhip64.so.7) and libpn2hip.so links the same SONAME, so loading it after torch binds it
to torch's HIP runtime — one runtime per process, torch's streams and allocations are valid
inside the library.
"""
import ctypes
import os

import torch

from . import _header

_HERE = os.path.dirname(os.path.abspath(__file__))
# PN2HIP_LIB: an alternative build of the same ABI (A/B measurements in tools/)
LIB_PATH = os.environ.get("PN2HIP_LIB") or os.path.join(_HERE, "libpn2hip.so")

ABI = _header.load(os.path.join(os.path.dirname(_HERE), "include"))
globals().update(ABI.constants)  # every PN2_* #define of the headers
POOL_MODES = {name[len("PN2_POOL_"):].lower(): mode for name, mode in ABI.constants.items()
              if name.startswith("PN2_POOL_") and name != "PN2_POOL_NONE"}
MlpLayer = ABI.structs["pn2_mlp_layer"]
SaLayer = ABI.structs["pn2_sa_layer"]
FpLayer = ABI.structs["pn2_fp_layer"]
AttnLayer = ABI.structs["pn2_attn_layer"]
AdamSlot = ABI.structs["pn2_adam_slot"]
SIGNATURES = ABI.functions  # name -> (restype, argtypes)


class InvalidArgumentError(ValueError):
    """Raised where the reference's OP_REQUIRES raises tf.errors.InvalidArgumentError."""


class Pn2RuntimeError(RuntimeError):
    """A HIP launch error reported by the C ABI."""


_lib = None


def lib():
    """The loaded libpn2hip.so (raises if it was not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` (make -C pointcloud-segmentation-attention_amd/csrc). "
                "pn2hip has no CPU fallback.")
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc, op):
    if rc == 0:
        return
    if rc == PN2_EINVAL:
        raise InvalidArgumentError(f"{op}: invalid argument")
    if rc == PN2_EFAULT:
        raise Pn2RuntimeError(f"{op}: an earlier sampler launch reported a device fault "
                              "(its indices are not trustworthy; see pn2_fault_status)")
    msg = lib().pn2_strerror(rc)
    raise Pn2RuntimeError(f"{op}: HIP error {rc}: {msg.decode() if msg else '?'}")


def check_device_faults(device=None):
    """Synchronise `device` and raise if a sampler launch stored a device fault code
    (include/pn2hip.h pn2_fault_status); clears the code."""
    torch.cuda.synchronize(device)
    code = lib().pn2_fault_status(1)
    if code:
        raise Pn2RuntimeError(f"device fault {code} reported by a sampler launch "
                              "(PN2_FAULT_FPS_POLL = 1: a cold wave's wait timed out)")


def stream_of(t):
    """hipStream_t handle of torch's current stream on t's device."""
    return torch.cuda.current_stream(t.device).cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def device_tensor(t, name, dtype):
    """Validate an op input: a GPU tensor of the reference dtype, made contiguous."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if t.device.type != "cuda":
        raise RuntimeError(
            f"{name} is on {t.device}: pn2hip ops run on the MI355X only (no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    return t.contiguous()


def aligned_device_tensor(t, name, dtype):
    """device_tensor for an argument whose C function demands 16-byte alignment (the attention
    reductions, include/pn2hip.h): a contiguous view at an odd offset into a larger buffer is
    copied to a fresh allocation. Arguments whose kernels have a scalar path use device_tensor
    and stay where they are."""
    t = device_tensor(t, name, dtype)
    return t.clone() if t.data_ptr() % 16 else t
