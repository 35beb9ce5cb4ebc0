"""ctypes binding of ``libminitorch_hip.so`` (C ABI declared in ``include/minitorch_hip.h``).

This is the MI355X counterpart of the reference's ctypes loading block
(reference ``minitorch/cuda_kernel_ops.py:25-29``): one library, located next to
this file rather than relative to the CWD, with every ``argtypes`` declared once.
There is no fallback: if the library is missing the first call raises.

Device buffers are torch tensors (PyTorch-ROCm is used for memory, streams and
``torch.distributed`` only); every computation goes through the HIP kernels.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Sequence

_HERE = os.path.dirname(os.path.abspath(__file__))
# MT_HIP_LIB: another build of the library (diagnostics: _lib/diag/libminitorch_hip_diag.so,
# `make DIAG=1`, which adds the A/B kernel policies) for tests and scripts; the package
# default is the product library
LIB_PATH = os.environ.get("MT_HIP_LIB") or os.path.join(_HERE, "_lib", "libminitorch_hip.so")

MT_F32 = 0
MT_BF16 = 1
# storage formats of a quantised KV cache (kv_dtype of the mt_*_kvq / *_quant entry points)
MT_KV_BF16 = 1
MT_KV_FP8 = 2

_lib = None
_allow_missing = False  # use_library(path, allow_missing=True): an older build may lack the newest entry points

_i64 = ctypes.c_int64
_int = ctypes.c_int
_vp = ctypes.c_void_p
_fp = ctypes.POINTER(ctypes.c_float)
_i64p = ctypes.POINTER(ctypes.c_int64)
_ip = ctypes.POINTER(ctypes.c_int)
_vpp = ctypes.POINTER(ctypes.c_void_p)

# name -> (restype, argtypes); mirrors include/minitorch_hip.h
_PROTOS = {
    "mt_last_error": (ctypes.c_char_p, []),
    "mt_abi_version": (_int, []),
    "mt_flash_set_kernel_policy": (_int, [_int]),
    "mt_flash_get_kernel_policy": (_int, []),
    "mt_scratch_bytes": (_i64, []),
    "mt_scratch_release": (_int, []),
    "mt_flash_attn_fwd": (_int, [_int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64,
                                 _i64p, _i64p, _i64p, _i64p, _vp]),
    "mt_flash_attn_fwd_varlen": (_int, [_int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64,
                                        _i64, _i64p, _i64p, _i64p, _i64p, _vp, _vp]),
    "mt_flash_attn_bwd_workspace_bytes": (_i64, [_i64, _i64, _i64, _i64]),
    "mt_flash_attn_bwd": (_int, [_int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                 _i64, _i64, _i64, _i64, _i64p, _vp, _vp]),
    "mt_flash_attn_bwd_varlen": (_int, [_int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                        _i64, _i64, _i64, _i64, _i64p, _vp, _vp, _vp]),
    "mt_flash_attn_bwd_v3": (_int, [_int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                    _i64, _i64, _i64, _i64, _i64p, _vp, _vp, _i64, _vp]),
    "mt_flash_attn_decode_splits": (_int, [_int, _i64, _i64, _i64, _i64, _i64, _i64p, _i64p]),
    "mt_flash_attn_decode_workspace_bytes": (_i64, [_int, _i64, _i64, _i64, _i64, _i64]),
    "mt_flash_attn_decode": (_int, [_int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64,
                                    _i64p, _i64p, _i64p, _i64p, _vp, _vp, _i64, _vp]),
    "mt_flash_attn_decode_gqa_splits": (_int, [_int, _i64, _i64, _i64, _i64, _i64, _i64, _i64p, _i64p]),
    "mt_flash_attn_decode_gqa_workspace_bytes": (_i64, [_int, _i64, _i64, _i64, _i64, _i64, _i64]),
    "mt_flash_attn_decode_gqa": (_int, [_int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64,
                                        _i64p, _i64p, _i64p, _i64p, _vp, _vp, _i64, _vp]),
    "mt_flash_attn_extend_plan": (_int, [_int, _i64, _i64, _i64, _i64, _i64, _i64, _i64p, _i64p]),
    "mt_flash_attn_extend": (_int, [_int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64,
                                    _i64p, _i64p, _i64p, _i64p, _vp, _vp, _vp]),
    "mt_kv_cache_append": (_int, [_int, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64,
                                  _i64p, _i64p, _i64p, _i64p, _vp, _vp]),
    "mt_flash_attn_decode_kvq_splits": (_int, [_int, _i64, _i64, _i64, _i64, _i64, _i64, _i64p, _i64p]),
    "mt_flash_attn_decode_kvq_workspace_bytes": (_i64, [_int, _i64, _i64, _i64, _i64, _i64, _i64]),
    "mt_flash_attn_decode_kvq": (_int, [_int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64,
                                        _i64, _i64, _i64p, _i64p, _i64p, _i64p, _vp, _vp, _i64, _vp]),
    "mt_flash_attn_extend_kvq_plan": (_int, [_int, _i64, _i64, _i64, _i64, _i64, _i64, _i64p, _i64p]),
    "mt_flash_attn_extend_kvq": (_int, [_int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64,
                                        _i64, _i64, _i64p, _i64p, _i64p, _i64p, _vp, _vp, _vp]),
    "mt_kv_cache_append_quant": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64,
                                        _i64p, _i64p, _i64p, _i64p, _vp, _vp]),
    "mt_kv_cache_dequant": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64,
                                   _i64p, _i64p, _i64p, _i64p, _vp, _vp]),
    "mt_flash_attn_decode_paged_splits": (_int, [_int, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64p, _i64p]),
    "mt_flash_attn_decode_paged_workspace_bytes": (_i64, [_int, _i64, _i64, _i64, _i64, _i64, _i64, _i64]),
    "mt_flash_attn_decode_paged": (_int, [_int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64,
                                          _i64, _i64, _i64, _i64p, _i64p, _i64p, _i64p, _vp, _vp, _vp, _i64, _vp]),
    "mt_flash_attn_extend_paged_plan": (_int, [_int, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64p, _i64p]),
    "mt_flash_attn_extend_paged": (_int, [_int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64,
                                          _i64, _i64, _i64, _i64p, _i64p, _i64p, _i64p, _vp, _vp, _vp, _vp]),
    "mt_kv_cache_append_paged": (_int, [_int, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i64,
                                        _i64p, _i64p, _i64p, _i64p, _vp, _vp, _vp, _vp]),
    "mt_kv_cache_gather_paged": (_int, [_int, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64,
                                        _i64p, _i64p, _i64p, _i64p, _vp, _vp, _vp]),
    "mt_select_token": (_int, [_vp, _i64, _i64, _i64, ctypes.c_float, _i64, ctypes.c_uint64, _vp, _i64,
                               _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    "mt_select_token_p": (_int, [_vp, _i64, _i64, _i64, ctypes.c_float, _i64, ctypes.c_float, ctypes.c_float,
                                 ctypes.c_uint64, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    "mt_spec_accept_p": (_int, [_vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, ctypes.c_float, _i64, ctypes.c_float,
                                ctypes.c_float, ctypes.c_uint64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                _vp, _i64, _i64, _vp, _i64, _vp, _vp]),
    "mt_spec_draft": (_int, [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    "mt_spec_accept": (_int, [_vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, ctypes.c_float, _i64, ctypes.c_uint64,
                              _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _i64, _vp,
                              _vp]),
    "mt_rope": (_int, [_int, _int, _vp, _vp, _i64, _i64p, _i64p, _vp, _vp, _i64, _i64p, _i64p,
                       _i64, _i64, _i64, _vp, _vp, _i64, _vp, _vp]),
    "mt_attn_softmax_fw": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64p, _int, _vp]),
    "mt_attn_softmax_bw": (_int, [_vp, _vp, _vp, _i64, _i64, _vp]),
    "mt_layernorm_fw": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp]),
    "mt_bias_gelu_fw": (_int, [_vp, _vp, _vp, _i64, _i64, _vp]),
    "mt_bias_gelu_bw": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _vp]),
    "mt_dropout": (_int, [_vp, _vp, _i64, ctypes.c_float, ctypes.c_float, ctypes.c_uint64, _vp]),
    "mt_dropout_dseed": (_int, [_vp, _vp, _i64, ctypes.c_float, ctypes.c_float, _vp, _vp]),
    "mt_embedding_fw": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _vp]),
    "mt_embedding_bw": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _vp]),
    "mt_softmax_xent_fw": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _vp]),
    "mt_softmax_xent_bw": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp]),
    "mt_layernorm_bw_workspace_bytes": (_i64, [_i64, _i64]),
    "mt_layernorm_bw": (_int, [_vp] * 9 + [_i64, _i64, _vp, _vp]),
    "mt_tensor_map": (_int, [_int, _vp, _i64p, _i64p, _int, _vp, _i64p, _i64p, _int, _vp]),
    "mt_tensor_zip": (_int, [_int, _vp, _i64p, _i64p, _int, _vp, _i64p, _i64p, _int,
                             _vp, _i64p, _i64p, _int, _vp]),
    "mt_tensor_reduce": (_int, [_int, _vp, _i64p, _i64p, _vp, _i64p, _i64p, _int, _int,
                                ctypes.c_float, _vp]),
    "mt_matmul_f32": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64p, _i64p, _i64p, _vp]),
    "mt_rand_uniform": (_int, [_vp, _i64, ctypes.c_uint64, _vp]),
    "mt_adam_step": (_int, [_int, _vpp, _vpp, _vpp, _vpp, _i64p, ctypes.c_double, ctypes.c_double,
                            ctypes.c_double, ctypes.c_double, _vp]),
    "mt_adam_step_dstep": (_int, [_int, _vpp, _vpp, _vpp, _vpp, _i64p, ctypes.c_double, ctypes.c_double,
                                  ctypes.c_double, _vp, _vp]),
    "mt_set_gemm_backend": (None, [_int]),
    "mt_matmul_f32_plan": (_int, [_int, _i64, _i64, _i64, _i64, _i64p, _i64p, _i64p, _vp, _vp, _vp,
                                  ctypes.POINTER(ctypes.c_int32)]),
    "launch_attn_softmax": (None, [_fp, _fp, _int, _int, _int, _int, ctypes.c_bool, _vp]),
    "launch_attn_softmax_bw": (None, [_fp, _fp, _int, _int, _vp]),
    "launch_layernorm": (None, [_fp] * 6 + [_int, _int, _vp]),
    "launch_layernorm_bw": (None, [_fp] * 9 + [_int, _int, _vp, _vp]),
    "tensorMap": (None, [_fp, _ip, _ip, _int, _fp, _ip, _ip, _int, _int, _int]),
    "tensorZip": (None, [_fp, _ip, _ip, _int, _int, _fp, _ip, _ip, _int, _int,
                         _fp, _ip, _ip, _int, _int, _int]),
    "tensorReduce": (None, [_fp, _ip, _ip, _int, _fp, _ip, _ip, _int, ctypes.c_float, _int, _int]),
    "MatrixMultiply": (None, [_fp, _ip, _ip, _fp, _ip, _ip, _fp, _ip, _ip, _int, _int, _int]),
    "launch_flashattention_forward": (None, [_fp] * 6 + [_int] * 4),
    "launch_flashattention_backward": (None, [_fp] * 10 + [_int] * 4),
    "launch_flashattention_forward_causal": (None, [_fp] * 6 + [_int] * 4),
    "launch_flashattention_backward_causal": (None, [_fp] * 10 + [_int] * 4),
}


def lib() -> ctypes.CDLL:
    """Load the HIP library (raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `make -C {os.path.dirname(_HERE)}` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        # One HIP runtime per process: torch's. Device buffers and streams are torch's, and
        # loaded first the library would bind /opt/rocm's libamdhip64 beside torch's bundled
        # one, which on some boxes then reports "no ROCm-capable device" for every call
        # (scripts/probe_runtime.py). With torch imported first, the library's libamdhip64
        # dependency resolves (by soname) to the runtime torch already mapped.
        try:
            import torch  # noqa: F401
        except ImportError:  # plain C-ABI use without torch: the library's own runtime
            pass
        l = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _PROTOS.items():
            fn = getattr(l, name, None)
            if fn is None:
                if _allow_missing:
                    continue
                raise AttributeError(f"{LIB_PATH} lacks {name}: rebuild it")
            fn.restype = res
            fn.argtypes = args
        _lib = l
        _bind_fast(l)
    return _lib


fast = None  # the _mtfast extension bound to the loaded library (None: the ops use ctypes)


def _bind_fast(l: ctypes.CDLL) -> None:
    """Hand the generic entry points' addresses of the loaded library to the _mtfast CPython
    extension (csrc/mtfast.c: tuples in, no ctypes marshalling), when it was built."""
    global fast
    try:
        from . import _mtfast
    except ImportError:
        fast = None
        return
    addr = lambda f: ctypes.cast(f, ctypes.c_void_p).value  # noqa: E731
    _mtfast.bind(addr(l.mt_tensor_map), addr(l.mt_tensor_zip), addr(l.mt_tensor_reduce), addr(l.mt_matmul_f32))
    fast = _mtfast


def use_library(path: str, allow_missing: bool = False) -> ctypes.CDLL:
    """Load a different build of the library (diagnostics only: scripts/ablate*.py load
    ``_lib/diag/libminitorch_hip_diag.so``, built by ``make DIAG=1``). The package itself
    always loads LIB_PATH. allow_missing: an entry point the build lacks (an older build, for an
    A/B against it) is left unbound, ``hasattr(lib(), name)`` tells, instead of being an error."""
    global _lib, LIB_PATH, _allow_missing
    if _lib is not None:
        raise RuntimeError("use_library() must run before the first lib() call")
    LIB_PATH = path
    _allow_missing = bool(allow_missing)
    return lib()


def set_policy(policy: int) -> None:
    """Select a kernel policy for A/B timing (mt_flash_set_kernel_policy; raises for an
    id the library rejects)."""
    check(lib().mt_flash_set_kernel_policy(int(policy)), "mt_flash_set_kernel_policy")


class policy:
    """``with _hip.policy(p): ...`` runs the block under kernel policy p, then restores
    the previous one."""

    def __init__(self, p: int):
        self.p = int(p)

    def __enter__(self):
        self.prev = lib().mt_flash_get_kernel_policy()
        set_policy(self.p)
        return self

    def __exit__(self, *exc):
        set_policy(self.prev)
        return False


def register(name: str, restype, argtypes) -> None:
    """Declare an additional export (used by the companion-kernel modules)."""
    _PROTOS[name] = (restype, argtypes)
    if _lib is not None:
        fn = getattr(_lib, name)
        fn.restype = restype
        fn.argtypes = argtypes


def check(status: int, what: str) -> None:
    if status != 0:
        msg = lib().mt_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed: {msg}")


# ---- torch plumbing -------------------------------------------------------------
def _torch():
    import torch
    return torch


def stream_ptr(device=None) -> int:
    """The current torch stream of `device` (default: the current device) as a raw
    hipStream_t. Uses the raw-stream accessor when present (no Stream object per call)."""
    torch = _torch()
    raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
    if raw is not None and (device is None or isinstance(device, int)):
        return raw(torch.cuda.current_device() if device is None else device)
    return torch.cuda.current_stream(device).cuda_stream


def dtype_code(t) -> int:
    torch = _torch()
    if t.dtype == torch.float32:
        return MT_F32
    if t.dtype == torch.bfloat16:
        return MT_BF16
    raise TypeError(f"unsupported dtype {t.dtype} (float32 or bfloat16)")


def strides3(t) -> ctypes.Array:
    """(batch, head, seq) element strides of a [B, H, N, d] tensor with unit-stride d."""
    if t.dim() != 4:
        raise ValueError(f"expected a 4-D [B,H,N,d] tensor, got shape {tuple(t.shape)}")
    if t.stride(3) != 1 and t.shape[3] != 1:
        raise ValueError("the head dimension must be unit-stride")
    return (ctypes.c_int64 * 3)(t.stride(0), t.stride(1), t.stride(2))


def _check_dev(*ts) -> None:
    for t in ts:
        if not t.is_cuda:
            raise ValueError("HIP flash attention needs device (cuda) tensors")


def _kv_arg(kv_len, B, device):
    """kv_len as the C ABI takes it: a device int32 [B] (None stays None)."""
    if kv_len is None:
        return None
    torch = _torch()
    kv = torch.as_tensor(kv_len, device=device).to(torch.int32).contiguous()
    if kv.shape != (B,):
        raise ValueError(f"kv_len must have shape ({B},), got {tuple(kv.shape)}")
    return kv


def flash_fwd(q, k, v, causal: bool = False, out=None, m=None, l=None, stream: Optional[int] = None,
              kv_len=None, out_dtype=None):
    """Device-pointer forward on torch tensors [B,H,N,d] (fp32 or bf16, any strides
    with unit-stride d). Returns (O, m, l); O has q's dtype, m/l are fp32 [B,H,N].
    kv_len: optional [B] valid-key counts (key padding: keys >= kv_len[b] are masked,
    mt_flash_attn_fwd_varlen). out_dtype=torch.float32 with bf16 inputs (or an fp32 `out`):
    the bf16 kernels write O in fp32, without its final bf16 rounding (MT_BF16_F32OUT)."""
    torch = _torch()
    _check_dev(q, k, v)
    B, H, N, d = q.shape
    if k.shape != q.shape or v.shape != q.shape:
        raise ValueError(f"q/k/v shapes differ: {tuple(q.shape)} {tuple(k.shape)} {tuple(v.shape)}")
    if not (q.dtype == k.dtype == v.dtype):
        raise TypeError("q/k/v dtypes differ")
    code = dtype_code(q)
    f32o = q.dtype == torch.bfloat16 and (out_dtype == torch.float32 or
                                          (out is not None and out.dtype == torch.float32))
    if out is None:
        out = torch.empty_like(q, dtype=torch.float32 if f32o else q.dtype,
                               memory_format=torch.contiguous_format)
    if f32o:
        code = 2  # MT_BF16_F32OUT
    if m is None:
        m = torch.empty((B, H, N), dtype=torch.float32, device=q.device)
    if l is None:
        l = torch.empty((B, H, N), dtype=torch.float32, device=q.device)
    st = stream_ptr(q.device) if stream is None else stream
    kv = _kv_arg(kv_len, B, q.device)
    if kv is None:
        check(lib().mt_flash_attn_fwd(code, int(causal), q.data_ptr(), k.data_ptr(),
                                      v.data_ptr(), out.data_ptr(), m.data_ptr(), l.data_ptr(),
                                      B, H, N, d, strides3(q), strides3(k), strides3(v),
                                      strides3(out), st), "mt_flash_attn_fwd")
    else:
        check(lib().mt_flash_attn_fwd_varlen(code, int(causal), q.data_ptr(), k.data_ptr(),
                                             v.data_ptr(), out.data_ptr(), m.data_ptr(), l.data_ptr(),
                                             B, H, N, d, strides3(q), strides3(k), strides3(v),
                                             strides3(out), kv.data_ptr(), st),
              "mt_flash_attn_fwd_varlen")
    return out, m, l


def flash_bwd(q, k, v, o, do, m, l, causal: bool = False, dq=None, dk=None, dv=None,
              workspace=None, stream: Optional[int] = None, kv_len=None):
    """Device-pointer backward. Returns (dQ, dK, dV) in q's dtype. kv_len: as flash_fwd."""
    torch = _torch()
    _check_dev(q, k, v, o, do, m, l)
    B, H, N, d = q.shape
    dq = torch.empty_like(q, memory_format=torch.contiguous_format) if dq is None else dq
    dk = torch.empty_like(k, memory_format=torch.contiguous_format) if dk is None else dk
    dv = torch.empty_like(v, memory_format=torch.contiguous_format) if dv is None else dv
    if workspace is None:
        nbytes = lib().mt_flash_attn_bwd_workspace_bytes(B, H, N, d)
        workspace = torch.empty(nbytes // 4, dtype=torch.float32, device=q.device)
    m = m.contiguous().float()
    l = l.contiguous().float()
    strides = (ctypes.c_int64 * 24)()
    for i, t in enumerate((q, k, v, o, do, dq, dk, dv)):
        s = strides3(t)
        strides[3 * i:3 * i + 3] = list(s)
    st = stream_ptr(q.device) if stream is None else stream
    kv = _kv_arg(kv_len, B, q.device)
    args = (dtype_code(q), int(causal), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
            do.data_ptr(), m.data_ptr(), l.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
            B, H, N, d, strides)
    # the size-checked entry (ABI 3): a workspace the caller sized too small is an error
    check(lib().mt_flash_attn_bwd_v3(*args, None if kv is None else kv.data_ptr(),
                                     workspace.data_ptr(), workspace.numel() * workspace.element_size(),
                                     st), "mt_flash_attn_bwd_v3")
    return dq, dk, dv


def _decode_code(q, out, out_dtype) -> int:
    torch = _torch()
    code = dtype_code(q)
    if q.dtype == torch.bfloat16 and (out_dtype == torch.float32 or
                                      (out is not None and out.dtype == torch.float32)):
        code = 2  # MT_BF16_F32OUT
    return code


def decode_splits(dtype: int, B: int, H: int, Nq: int, Nk: int, d: int, Hkv: Optional[int] = None):
    """(splits, span_keys, tile_keys) of mt_flash_attn_decode[_gqa] at these sizes (dtype: an MT_*
    code): how many workgroups share the keys of one (batch, head), the keys each takes and the
    keys one wave takes per inner step. A function of the sizes only. Hkv: the caches' heads
    (None: H)."""
    span, tile = ctypes.c_int64(0), ctypes.c_int64(0)
    n = lib().mt_flash_attn_decode_gqa_splits(dtype, B, H, H if Hkv is None else Hkv, Nq, Nk, d,
                                              ctypes.byref(span), ctypes.byref(tile))
    if n <= 0:
        raise ValueError(lib().mt_last_error().decode(errors="replace"))
    return n, span.value, tile.value


def decode_workspace_bytes(dtype: int, B: int, H: int, Nq: int, Nk: int, d: int, Hkv: Optional[int] = None) -> int:
    n = lib().mt_flash_attn_decode_gqa_workspace_bytes(dtype, B, H, H if Hkv is None else Hkv, Nq, Nk, d)
    if n < 0:
        raise ValueError(lib().mt_last_error().decode(errors="replace"))
    return int(n)


def flash_decode(q, k_cache, v_cache, kv_len=None, causal: bool = True, out=None, m=None, l=None,
                 workspace=None, out_dtype=None, stream: Optional[int] = None):
    """Decode attention (mt_flash_attn_decode_gqa): q [B,H,Nq,d] (Nq <= 8, the last Nq positions
    of each row) against the caches [B,Hkv,Nk,d] (any strides with unit-stride d; Hkv divides H,
    query head h reads kv head h // (H // Hkv)), of which the first kv_len[b] rows are visible
    (None: all Nk). Returns (O, m, l); m, l fp32 [B,H,Nq]. workspace: a device buffer of at least
    decode_workspace_bytes (allocated when None)."""
    torch = _torch()
    _check_dev(q, k_cache, v_cache)
    B, H, Nq, d = q.shape
    Hkv, Nk = k_cache.shape[1], k_cache.shape[2]
    if k_cache.shape != (B, Hkv, Nk, d) or v_cache.shape != k_cache.shape:
        raise ValueError(f"cache shapes {tuple(k_cache.shape)} {tuple(v_cache.shape)} do not match q {tuple(q.shape)}")
    if Hkv <= 0 or H % Hkv:
        raise ValueError(f"the caches' {Hkv} heads do not divide q's {H} heads")
    if not (q.dtype == k_cache.dtype == v_cache.dtype):
        raise TypeError("q/k_cache/v_cache dtypes differ")
    code = _decode_code(q, out, out_dtype)
    if out is None:
        out = torch.empty((B, H, Nq, d), dtype=torch.float32 if code == 2 else q.dtype, device=q.device)
    if m is None:
        m = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
    if l is None:
        l = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
    need = lib().mt_flash_attn_decode_gqa_workspace_bytes(code, B, H, Hkv, Nq, Nk, d)
    if workspace is None and need > 0:
        workspace = torch.empty(need // 4, dtype=torch.float32, device=q.device)
    kv = _kv_arg(kv_len, B, q.device)
    st = stream_ptr(q.device) if stream is None else stream
    check(lib().mt_flash_attn_decode_gqa(
        code, int(causal), q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), out.data_ptr(),
        m.data_ptr(), l.data_ptr(), B, H, Hkv, Nq, Nk, d, strides3(q), strides3(k_cache), strides3(v_cache),
        strides3(out), None if kv is None else kv.data_ptr(),
        None if workspace is None else workspace.data_ptr(),
        0 if workspace is None else workspace.numel() * workspace.element_size(), st),
        "mt_flash_attn_decode_gqa")
    return out, m, l


def extend_plan(dtype: int, B: int, H: int, Nq: int, Nk: int, d: int, Hkv: Optional[int] = None):
    """(kernel id, block_queries, tile_keys) of mt_flash_attn_extend at these sizes (dtype: an MT_*
    code): the instantiation it launches, the query rows one workgroup owns and the keys of one
    inner tile. A function of the sizes only; no device call. Hkv: the caches' heads (None: H)."""
    bq, bk = ctypes.c_int64(0), ctypes.c_int64(0)
    kid = lib().mt_flash_attn_extend_plan(dtype, B, H, H if Hkv is None else Hkv, Nq, Nk, d,
                                          ctypes.byref(bq), ctypes.byref(bk))
    if kid < 0:
        raise ValueError(lib().mt_last_error().decode(errors="replace"))
    return kid, bq.value, bk.value


def flash_extend(q, k_cache, v_cache, kv_len=None, q_len=None, causal: bool = True, out=None, m=None, l=None,
                 out_dtype=None, stream: Optional[int] = None):
    """Extend attention (mt_flash_attn_extend): q [B,H,Nq,d], any 1 <= Nq <= Nk new rows at the end
    of each row, of which the first q_len[b] are real (None: all Nq; the batch is right-padded),
    against the caches [B,Hkv,Nk,d] (any strides with unit-stride d; Hkv divides H), which hold
    kv_len[b] rows after the new ones were appended (None: Nk). Query i < q_len[b] sits at position
    kv_len[b] - q_len[b] + i. Returns (O, m, l); m, l fp32 [B,H,Nq]; a query >= q_len[b] or without
    a visible key gets (0, -inf, 0). One launch, no workspace."""
    torch = _torch()
    _check_dev(q, k_cache, v_cache)
    B, H, Nq, d = q.shape
    Hkv, Nk = k_cache.shape[1], k_cache.shape[2]
    if k_cache.shape != (B, Hkv, Nk, d) or v_cache.shape != k_cache.shape:
        raise ValueError(f"cache shapes {tuple(k_cache.shape)} {tuple(v_cache.shape)} do not match q {tuple(q.shape)}")
    if Hkv <= 0 or H % Hkv:
        raise ValueError(f"the caches' {Hkv} heads do not divide q's {H} heads")
    if not (q.dtype == k_cache.dtype == v_cache.dtype):
        raise TypeError("q/k_cache/v_cache dtypes differ")
    code = _decode_code(q, out, out_dtype)
    if out is None:
        out = torch.empty((B, H, Nq, d), dtype=torch.float32 if code == 2 else q.dtype, device=q.device)
    if m is None:
        m = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
    if l is None:
        l = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
    kv = _kv_arg(kv_len, B, q.device)
    ql = _kv_arg(q_len, B, q.device)
    st = stream_ptr(q.device) if stream is None else stream
    check(lib().mt_flash_attn_extend(
        code, int(causal), q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), out.data_ptr(),
        m.data_ptr(), l.data_ptr(), B, H, Hkv, Nq, Nk, d, strides3(q), strides3(k_cache), strides3(v_cache),
        strides3(out), None if kv is None else kv.data_ptr(), None if ql is None else ql.data_ptr(), st),
        "mt_flash_attn_extend")
    return out, m, l


def kv_cache_append(k_new, v_new, k_cache, v_cache, pos, stream: Optional[int] = None) -> None:
    """Copy the new rows k_new / v_new [B,H,Nq,d] into the caches [B,H,Nmax,d] at rows
    pos[b] .. pos[b] + Nq - 1 (pos: [B] int32 on the device; rows past the capacity are dropped).
    H is the caches' head count (the kv heads of a grouped-query model)."""
    torch = _torch()
    _check_dev(k_new, v_new, k_cache, v_cache)
    B, H, Nq, d = k_new.shape
    Nmax = k_cache.shape[2]
    if v_new.shape != k_new.shape or k_cache.shape != (B, H, Nmax, d) or v_cache.shape != k_cache.shape:
        raise ValueError("kv_cache_append: shapes do not match")
    if not (k_new.dtype == v_new.dtype == k_cache.dtype == v_cache.dtype):
        raise TypeError("kv_cache_append: dtypes differ")
    p = _kv_arg(pos, B, k_new.device)
    st = stream_ptr(k_new.device) if stream is None else stream
    check(lib().mt_kv_cache_append(
        dtype_code(k_new), k_new.data_ptr(), v_new.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
        B, H, Nq, Nmax, d, strides3(k_new), strides3(v_new), strides3(k_cache), strides3(v_cache),
        p.data_ptr(), st), "mt_kv_cache_append")


# ---- quantised KV cache (mt_kv_cache_append_quant / mt_flash_attn_decode_kvq / mt_kv_cache_dequant) ----
def kv_code(cache) -> int:
    """The kv_dtype code of a quantised cache tensor: torch.bfloat16 -> MT_KV_BF16, torch.uint8
    (one e4m3 code per byte) -> MT_KV_FP8."""
    torch = _torch()
    if cache.dtype == torch.bfloat16:
        return MT_KV_BF16
    if cache.dtype == torch.uint8:
        return MT_KV_FP8
    raise TypeError(f"a quantised cache is torch.bfloat16 or torch.uint8 (e4m3 codes), got {cache.dtype}")


def _kvq_caches(name, k_cache, v_cache, k_scale, v_scale, B, d):
    """Checks shared by the three entry points; returns (code, Hkv, N, k_scale ptr, v_scale ptr)."""
    torch = _torch()
    code = kv_code(k_cache)
    if k_cache.dim() != 4 or v_cache.shape != k_cache.shape or v_cache.dtype != k_cache.dtype:
        raise ValueError(f"{name}: the caches must be two [B,Hkv,N,d] tensors of one dtype")
    _, Hkv, N, dc = k_cache.shape
    if k_cache.shape[0] != B or dc != d:
        raise ValueError(f"{name}: cache shape {tuple(k_cache.shape)} does not match (B, d) = ({B}, {d})")
    if d > 1 and (k_cache.stride(3) != 1 or v_cache.stride(3) != 1):
        raise ValueError(f"{name}: the caches need a unit-stride last dim")
    if code == MT_KV_BF16:
        return code, Hkv, N, None, None
    for nm, s in (("k_scale", k_scale), ("v_scale", v_scale)):
        if s is None:
            raise ValueError(f"{name}: an fp8 cache needs {nm}")
        if (not s.is_cuda or s.dtype != torch.float32 or tuple(s.shape) != (B, Hkv, N) or not s.is_contiguous()):
            raise ValueError(f"{name}: {nm} must be a contiguous device float32 [{B}, {Hkv}, {N}] tensor")
    return code, Hkv, N, k_scale.data_ptr(), v_scale.data_ptr()


def decode_kvq_splits(kv_dtype: int, B: int, H: int, Nq: int, Nk: int, d: int, Hkv: Optional[int] = None):
    """(splits, span_keys, tile_keys) of mt_flash_attn_decode_kvq: decode_splits' answer for a bf16
    cache at the same sizes, whatever the format (both are read in chunks of 8 elements)."""
    span, tile = ctypes.c_int64(0), ctypes.c_int64(0)
    n = lib().mt_flash_attn_decode_kvq_splits(kv_dtype, B, H, H if Hkv is None else Hkv, Nq, Nk, d,
                                              ctypes.byref(span), ctypes.byref(tile))
    if n <= 0:
        raise ValueError(lib().mt_last_error().decode(errors="replace"))
    return n, span.value, tile.value


def decode_kvq_workspace_bytes(kv_dtype: int, B: int, H: int, Nq: int, Nk: int, d: int,
                               Hkv: Optional[int] = None) -> int:
    n = lib().mt_flash_attn_decode_kvq_workspace_bytes(kv_dtype, B, H, H if Hkv is None else Hkv, Nq, Nk, d)
    if n < 0:
        raise ValueError(lib().mt_last_error().decode(errors="replace"))
    return int(n)


def kv_cache_append_quant(k_new, v_new, k_cache, v_cache, pos, k_scale=None, v_scale=None,
                          stream: Optional[int] = None) -> None:
    """Quantise the fp32 new rows k_new / v_new [B,Hkv,Nq,d] into the caches [B,Hkv,Nmax,d]
    (torch.bfloat16, or torch.uint8 e4m3 codes with the fp32 row scales k_scale / v_scale
    [B,Hkv,Nmax]) at rows pos[b] .. pos[b] + Nq - 1 (rows past the capacity are dropped)."""
    torch = _torch()
    _check_dev(k_new, v_new, k_cache, v_cache)
    B, Hkv, Nq, d = k_new.shape
    if v_new.shape != k_new.shape or k_new.dtype != torch.float32 or v_new.dtype != torch.float32:
        raise ValueError("kv_cache_append_quant: the new rows must be two float32 [B,Hkv,Nq,d] tensors")
    code, Hc, Nmax, ksp, vsp = _kvq_caches("kv_cache_append_quant", k_cache, v_cache, k_scale, v_scale, B, d)
    if Hc != Hkv:
        raise ValueError("kv_cache_append_quant: shapes do not match")
    p = _kv_arg(pos, B, k_new.device)
    st = stream_ptr(k_new.device) if stream is None else stream
    check(lib().mt_kv_cache_append_quant(
        code, k_new.data_ptr(), v_new.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), ksp, vsp,
        B, Hkv, Nq, Nmax, d, strides3(k_new), strides3(v_new), strides3(k_cache), strides3(v_cache),
        p.data_ptr(), st), "mt_kv_cache_append_quant")


def flash_decode_kvq(q, k_cache, v_cache, k_scale=None, v_scale=None, kv_len=None, causal: bool = True,
                     out=None, m=None, l=None, workspace=None, stream: Optional[int] = None):
    """Decode attention on a quantised cache (mt_flash_attn_decode_kvq): flash_decode's contract
    with an fp32 q [B,H,Nq,d], fp32 (O, m, l) and the caches [B,Hkv,Nk,d] as torch.bfloat16, or
    torch.uint8 e4m3 codes with the fp32 row scales [B,Hkv,Nk]. workspace: a device buffer of at
    least decode_kvq_workspace_bytes (allocated when None)."""
    torch = _torch()
    _check_dev(q, k_cache, v_cache)
    B, H, Nq, d = q.shape
    if q.dtype != torch.float32:
        raise TypeError("flash_decode_kvq takes float32 queries")
    code, Hkv, Nk, ksp, vsp = _kvq_caches("flash_decode_kvq", k_cache, v_cache, k_scale, v_scale, B, d)
    if Hkv <= 0 or H % Hkv:
        raise ValueError(f"the caches' {Hkv} heads do not divide q's {H} heads")
    if out is None:
        out = torch.empty((B, H, Nq, d), dtype=torch.float32, device=q.device)
    elif out.dtype != torch.float32:
        raise TypeError("flash_decode_kvq writes a float32 O")
    if m is None:
        m = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
    if l is None:
        l = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
    need = lib().mt_flash_attn_decode_kvq_workspace_bytes(code, B, H, Hkv, Nq, Nk, d)
    if workspace is None and need > 0:
        workspace = torch.empty(need // 4, dtype=torch.float32, device=q.device)
    kv = _kv_arg(kv_len, B, q.device)
    st = stream_ptr(q.device) if stream is None else stream
    check(lib().mt_flash_attn_decode_kvq(
        code, int(causal), q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), ksp, vsp, out.data_ptr(),
        m.data_ptr(), l.data_ptr(), B, H, Hkv, Nq, Nk, d, strides3(q), strides3(k_cache), strides3(v_cache),
        strides3(out), None if kv is None else kv.data_ptr(),
        None if workspace is None else workspace.data_ptr(),
        0 if workspace is None else workspace.numel() * workspace.element_size(), st),
        "mt_flash_attn_decode_kvq")
    return out, m, l


def extend_kvq_plan(kv_dtype: int, B: int, H: int, Nq: int, Nk: int, d: int, Hkv: Optional[int] = None):
    """(kernel id, block_queries, tile_keys) of mt_flash_attn_extend_kvq: extend_plan's answer for
    MT_F32 at the same sizes, whatever the format (the rows are staged as fp32)."""
    bq, bk = ctypes.c_int64(0), ctypes.c_int64(0)
    kid = lib().mt_flash_attn_extend_kvq_plan(kv_dtype, B, H, H if Hkv is None else Hkv, Nq, Nk, d,
                                              ctypes.byref(bq), ctypes.byref(bk))
    if kid < 0:
        raise ValueError(lib().mt_last_error().decode(errors="replace"))
    return kid, bq.value, bk.value


def flash_extend_kvq(q, k_cache, v_cache, k_scale=None, v_scale=None, kv_len=None, q_len=None, causal: bool = True,
                     out=None, m=None, l=None, stream: Optional[int] = None):
    """Extend attention on a quantised cache read in place (mt_flash_attn_extend_kvq): flash_extend's
    contract with an fp32 q [B,H,Nq,d], fp32 (O, m, l) and the caches [B,Hkv,Nk,d] as torch.bfloat16,
    or torch.uint8 e4m3 codes with the fp32 row scales [B,Hkv,Nk]. The bits are those of
    kv_cache_dequant followed by flash_extend. One launch, no workspace."""
    torch = _torch()
    _check_dev(q, k_cache, v_cache)
    B, H, Nq, d = q.shape
    if q.dtype != torch.float32:
        raise TypeError("flash_extend_kvq takes float32 queries")
    code, Hkv, Nk, ksp, vsp = _kvq_caches("flash_extend_kvq", k_cache, v_cache, k_scale, v_scale, B, d)
    if Hkv <= 0 or H % Hkv:
        raise ValueError(f"the caches' {Hkv} heads do not divide q's {H} heads")
    if out is None:
        out = torch.empty((B, H, Nq, d), dtype=torch.float32, device=q.device)
    elif out.dtype != torch.float32:
        raise TypeError("flash_extend_kvq writes a float32 O")
    if m is None:
        m = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
    if l is None:
        l = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
    kv = _kv_arg(kv_len, B, q.device)
    ql = _kv_arg(q_len, B, q.device)
    st = stream_ptr(q.device) if stream is None else stream
    check(lib().mt_flash_attn_extend_kvq(
        code, int(causal), q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), ksp, vsp, out.data_ptr(),
        m.data_ptr(), l.data_ptr(), B, H, Hkv, Nq, Nk, d, strides3(q), strides3(k_cache), strides3(v_cache),
        strides3(out), None if kv is None else kv.data_ptr(), None if ql is None else ql.data_ptr(), st),
        "mt_flash_attn_extend_kvq")
    return out, m, l


def kv_cache_dequant(k_cache, v_cache, k_scale=None, v_scale=None, kv_len=None, k_out=None, v_out=None,
                     stream: Optional[int] = None):
    """The fp32 values of the first kv_len[b] rows (None: all) of a quantised cache
    (mt_kv_cache_dequant) written to k_out / v_out [B,Hkv,Nk,d] float32 (allocated, uninitialised
    past those rows, when None); the other rows are neither read nor written. Returns them."""
    torch = _torch()
    _check_dev(k_cache, v_cache)
    B, d = k_cache.shape[0], k_cache.shape[3]
    code, Hkv, Nk, ksp, vsp = _kvq_caches("kv_cache_dequant", k_cache, v_cache, k_scale, v_scale, B, d)
    if k_out is None:
        k_out = torch.empty((B, Hkv, Nk, d), dtype=torch.float32, device=k_cache.device)
    if v_out is None:
        v_out = torch.empty((B, Hkv, Nk, d), dtype=torch.float32, device=k_cache.device)
    for t in (k_out, v_out):
        if t.dtype != torch.float32 or tuple(t.shape) != (B, Hkv, Nk, d):
            raise ValueError(f"kv_cache_dequant: outputs must be float32 [{B}, {Hkv}, {Nk}, {d}] tensors")
    kv = _kv_arg(kv_len, B, k_cache.device)
    st = stream_ptr(k_cache.device) if stream is None else stream
    check(lib().mt_kv_cache_dequant(
        code, k_cache.data_ptr(), v_cache.data_ptr(), ksp, vsp, k_out.data_ptr(), v_out.data_ptr(),
        B, Hkv, Nk, d, strides3(k_cache), strides3(v_cache), strides3(k_out), strides3(v_out),
        None if kv is None else kv.data_ptr(), st), "mt_kv_cache_dequant")
    return k_out, v_out


# ---- paged KV cache (mt_flash_attn_decode_paged / mt_kv_cache_append_paged / mt_kv_cache_gather_paged) ----
def _paged_pools(name, k_pool, v_pool, block_table, B):
    """Checks shared by the three entry points; returns (n_pages, Hkv, P, d, W). The pools are
    [n_pages,Hkv,P,d] views (any strides with unit-stride d), the table a dense device int32 [B,W]."""
    torch = _torch()
    _check_dev(k_pool, v_pool, block_table)
    if k_pool.dim() != 4 or v_pool.shape != k_pool.shape or v_pool.dtype != k_pool.dtype:
        raise ValueError(f"{name}: the pools must be two [n_pages,Hkv,P,d] tensors of one dtype")
    if block_table.dtype != torch.int32 or block_table.dim() != 2 or not block_table.is_contiguous():
        raise ValueError(f"{name}: the block table must be a contiguous device int32 [B,W] tensor")
    if block_table.shape[0] != B:
        raise ValueError(f"{name}: the block table has {block_table.shape[0]} rows, the batch {B}")
    n_pages, Hkv, P, d = k_pool.shape
    return n_pages, Hkv, P, d, block_table.shape[1]


def decode_paged_splits(dtype: int, B: int, H: int, Nq: int, W: int, P: int, d: int, Hkv: Optional[int] = None):
    """(splits, span_keys, tile_keys) of mt_flash_attn_decode_paged: decode_splits' answer at
    Nk = W * P. A function of the sizes only."""
    span, tile = ctypes.c_int64(0), ctypes.c_int64(0)
    n = lib().mt_flash_attn_decode_paged_splits(dtype, B, H, H if Hkv is None else Hkv, Nq, W, P, d,
                                                ctypes.byref(span), ctypes.byref(tile))
    if n <= 0:
        raise ValueError(lib().mt_last_error().decode(errors="replace"))
    return n, span.value, tile.value


def decode_paged_workspace_bytes(dtype: int, B: int, H: int, Nq: int, W: int, P: int, d: int,
                                 Hkv: Optional[int] = None) -> int:
    n = lib().mt_flash_attn_decode_paged_workspace_bytes(dtype, B, H, H if Hkv is None else Hkv, Nq, W, P, d)
    if n < 0:
        raise ValueError(lib().mt_last_error().decode(errors="replace"))
    return int(n)


def flash_decode_paged(q, k_pool, v_pool, block_table, kv_len=None, causal: bool = True, out=None, m=None,
                       l=None, workspace=None, out_dtype=None, stream: Optional[int] = None):
    """Decode attention on a paged cache (mt_flash_attn_decode_paged): flash_decode's contract with
    q [B,H,Nq,d] against the page pools [n_pages,Hkv,P,d] (any strides with unit-stride d) through
    block_table (device int32 [B,W]: key j of row b is row j % P of page block_table[b, j // P]).
    The first kv_len[b] of the W * P logical keys are visible (None: all). Returns (O, m, l).
    workspace: a device buffer of at least decode_paged_workspace_bytes (allocated when None)."""
    torch = _torch()
    _check_dev(q)
    B, H, Nq, d = q.shape
    n_pages, Hkv, P, dp, W = _paged_pools("flash_decode_paged", k_pool, v_pool, block_table, B)
    if dp != d:
        raise ValueError(f"pool shape {tuple(k_pool.shape)} does not match q {tuple(q.shape)}")
    if Hkv <= 0 or H % Hkv:
        raise ValueError(f"the pools' {Hkv} heads do not divide q's {H} heads")
    if not (q.dtype == k_pool.dtype == v_pool.dtype):
        raise TypeError("q/k_pool/v_pool dtypes differ")
    code = _decode_code(q, out, out_dtype)
    if out is None:
        out = torch.empty((B, H, Nq, d), dtype=torch.float32 if code == 2 else q.dtype, device=q.device)
    if m is None:
        m = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
    if l is None:
        l = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
    need = lib().mt_flash_attn_decode_paged_workspace_bytes(code, B, H, Hkv, Nq, W, P, d)
    if workspace is None and need > 0:
        workspace = torch.empty(need // 4, dtype=torch.float32, device=q.device)
    kv = _kv_arg(kv_len, B, q.device)
    st = stream_ptr(q.device) if stream is None else stream
    check(lib().mt_flash_attn_decode_paged(
        code, int(causal), q.data_ptr(), k_pool.data_ptr(), v_pool.data_ptr(), out.data_ptr(),
        m.data_ptr(), l.data_ptr(), B, H, Hkv, Nq, W, P, n_pages, d, strides3(q), strides3(k_pool),
        strides3(v_pool), strides3(out), block_table.data_ptr(), None if kv is None else kv.data_ptr(),
        None if workspace is None else workspace.data_ptr(),
        0 if workspace is None else workspace.numel() * workspace.element_size(), st),
        "mt_flash_attn_decode_paged")
    return out, m, l


def extend_paged_plan(dtype: int, B: int, H: int, Nq: int, W: int, P: int, d: int, Hkv: Optional[int] = None):
    """(kernel id, block_queries, tile_keys) of mt_flash_attn_extend_paged: extend_plan's answer at
    Nk = W * P. A function of the sizes only."""
    bq, bk = ctypes.c_int64(0), ctypes.c_int64(0)
    kid = lib().mt_flash_attn_extend_paged_plan(dtype, B, H, H if Hkv is None else Hkv, Nq, W, P, d,
                                                ctypes.byref(bq), ctypes.byref(bk))
    if kid < 0:
        raise ValueError(lib().mt_last_error().decode(errors="replace"))
    return kid, bq.value, bk.value


def flash_extend_paged(q, k_pool, v_pool, block_table, kv_len=None, q_len=None, causal: bool = True, out=None,
                       m=None, l=None, out_dtype=None, stream: Optional[int] = None):
    """Extend attention on a paged cache read in place (mt_flash_attn_extend_paged): flash_extend's
    contract with q [B,H,Nq,d] against the page pools [n_pages,Hkv,P,d] (any strides with unit-stride
    d) through block_table (device int32 [B,W]: key j of row b is row j % P of page
    block_table[b, j // P]). The first kv_len[b] of the W * P logical keys are visible (None: all).
    The bits are those of flash_extend on a contiguous cache holding the same rows. Returns (O, m, l).
    One launch, no workspace."""
    torch = _torch()
    _check_dev(q)
    B, H, Nq, d = q.shape
    n_pages, Hkv, P, dp, W = _paged_pools("flash_extend_paged", k_pool, v_pool, block_table, B)
    if dp != d:
        raise ValueError(f"pool shape {tuple(k_pool.shape)} does not match q {tuple(q.shape)}")
    if Hkv <= 0 or H % Hkv:
        raise ValueError(f"the pools' {Hkv} heads do not divide q's {H} heads")
    if not (q.dtype == k_pool.dtype == v_pool.dtype):
        raise TypeError("q/k_pool/v_pool dtypes differ")
    code = _decode_code(q, out, out_dtype)
    if out is None:
        out = torch.empty((B, H, Nq, d), dtype=torch.float32 if code == 2 else q.dtype, device=q.device)
    if m is None:
        m = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
    if l is None:
        l = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
    kv = _kv_arg(kv_len, B, q.device)
    ql = _kv_arg(q_len, B, q.device)
    st = stream_ptr(q.device) if stream is None else stream
    check(lib().mt_flash_attn_extend_paged(
        code, int(causal), q.data_ptr(), k_pool.data_ptr(), v_pool.data_ptr(), out.data_ptr(),
        m.data_ptr(), l.data_ptr(), B, H, Hkv, Nq, W, P, n_pages, d, strides3(q), strides3(k_pool),
        strides3(v_pool), strides3(out), block_table.data_ptr(), None if kv is None else kv.data_ptr(),
        None if ql is None else ql.data_ptr(), st),
        "mt_flash_attn_extend_paged")
    return out, m, l


def kv_cache_append_paged(k_new, v_new, k_pool, v_pool, block_table, pos, count=None,
                          stream: Optional[int] = None) -> None:
    """Copy the new rows k_new / v_new [B,Hkv,Nq,d] into the page pools [n_pages,Hkv,P,d] at the
    logical rows pos[b] .. pos[b] + count[b] - 1 of batch row b (pos, count: [B] int32 on the
    device; count None: Nq). Rows past the count, past W * P or in an unallocated page (a negative
    table entry) are dropped."""
    _check_dev(k_new, v_new)
    B, Hkv, Nq, d = k_new.shape
    n_pages, Hp, P, dp, W = _paged_pools("kv_cache_append_paged", k_pool, v_pool, block_table, B)
    if v_new.shape != k_new.shape or (Hp, dp) != (Hkv, d):
        raise ValueError("kv_cache_append_paged: shapes do not match")
    if not (k_new.dtype == v_new.dtype == k_pool.dtype):
        raise TypeError("kv_cache_append_paged: dtypes differ")
    p = _kv_arg(pos, B, k_new.device)
    cnt = _kv_arg(count, B, k_new.device)
    st = stream_ptr(k_new.device) if stream is None else stream
    check(lib().mt_kv_cache_append_paged(
        dtype_code(k_new), k_new.data_ptr(), v_new.data_ptr(), k_pool.data_ptr(), v_pool.data_ptr(),
        B, Hkv, Nq, W, P, n_pages, d, strides3(k_new), strides3(v_new), strides3(k_pool), strides3(v_pool),
        block_table.data_ptr(), p.data_ptr(), None if cnt is None else cnt.data_ptr(), st),
        "mt_kv_cache_append_paged")


def kv_cache_gather_paged(k_pool, v_pool, block_table, kv_len=None, k_out=None, v_out=None,
                          stream: Optional[int] = None):
    """The first kv_len[b] logical rows (None: all W * P) of every batch row of a paged cache
    (mt_kv_cache_gather_paged) written to the contiguous k_out / v_out [B,Hkv,W*P,d] (allocated,
    uninitialised past those rows, when None); the other rows are neither read nor written."""
    torch = _torch()
    B = block_table.shape[0]
    n_pages, Hkv, P, d, W = _paged_pools("kv_cache_gather_paged", k_pool, v_pool, block_table, B)
    Nk = W * P
    if k_out is None:
        k_out = torch.empty((B, Hkv, Nk, d), dtype=k_pool.dtype, device=k_pool.device)
    if v_out is None:
        v_out = torch.empty((B, Hkv, Nk, d), dtype=k_pool.dtype, device=k_pool.device)
    for t in (k_out, v_out):
        if t.dtype != k_pool.dtype or tuple(t.shape) != (B, Hkv, Nk, d):
            raise ValueError(f"kv_cache_gather_paged: outputs must be {k_pool.dtype} [{B}, {Hkv}, {Nk}, {d}] tensors")
    kv = _kv_arg(kv_len, B, k_pool.device)
    st = stream_ptr(k_pool.device) if stream is None else stream
    check(lib().mt_kv_cache_gather_paged(
        dtype_code(k_pool), k_pool.data_ptr(), v_pool.data_ptr(), k_out.data_ptr(), v_out.data_ptr(),
        B, Hkv, W, P, n_pages, d, strides3(k_pool), strides3(v_pool), strides3(k_out), strides3(v_out),
        block_table.data_ptr(), None if kv is None else kv.data_ptr(), st), "mt_kv_cache_gather_paged")
    return k_out, v_out


def rand_uniform(n: int, seed: int, out=None, stream: Optional[int] = None):
    """n draws of U[0,1) on the device (mt_rand_uniform: the counter-based hash of (seed, index));
    returns the fp32 [n] tensor (`out` when given: dense, n elements)."""
    torch = _torch()
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device="cuda")
    if not out.is_cuda or out.dtype != torch.float32 or out.numel() != n or not out.is_contiguous():
        raise ValueError(f"rand_uniform: out must be a contiguous device float32 tensor of {n} elements")
    st = stream_ptr(out.device) if stream is None else stream
    check(lib().mt_rand_uniform(out.data_ptr(), n, int(seed) & 0xFFFFFFFFFFFFFFFF, st), "mt_rand_uniform")
    return out


def _nucleus_entry(name: str, top_p: float, min_p: float):
    """(the entry `name`_p, True), or (the entry without the filters, False) where a library loaded
    by use_library(allow_missing=True) predates them and both are at their off values."""
    fn = getattr(lib(), name + "_p", None)
    if fn is not None:
        return fn, True
    if top_p == 1.0 and min_p == 0.0:
        return getattr(lib(), name), False
    raise RuntimeError(f"{LIB_PATH} lacks {name}_p (top_p / min_p): rebuild it")


def select_token(logits, temperature: float = 0.0, top_k: int = 0, seed: int = 0, seed_dev=None, eos_id=None,
                 out=None, out_i32=None, done=None, history=None, step_dev=None, stream: Optional[int] = None,
                 top_p: float = 1.0, min_p: float = 0.0):
    """The next token id of every row of logits (mt_select_token_p): a 2-D fp32 device view [B, V]
    with a unit-stride last dim and any row stride >= V (e.g. ``logits3d[:, -1]``, no copy).
    temperature 0: greedy (np.argmax's id); > 0: a draw from softmax(logits / temperature) over
    the top_k largest entries (0: all), cut further to the nucleus of mass top_p (1: off) and to
    the entries of at least min_p times the largest probability (0: off), with u the value
    rand_uniform writes at index b for `seed`. seed_dev: a device int64 [1] holding the seed
    instead (read when the kernel runs).
    Returns (out, out_i32): fp32 [B] and int32 [B] ids, allocated when not given. done: int32 [B]
    in/out, done[b] |= (id == eos_id). history: int32 [B, S] with step_dev an int32 [1] on the
    device: history[b, step_dev[0]] = id."""
    torch = _torch()
    _check_dev(logits)
    if logits.dim() != 2 or logits.dtype != torch.float32:
        raise ValueError(f"select_token takes a 2-D float32 [B, V] view, got {tuple(logits.shape)} {logits.dtype}")
    B, V = logits.shape
    if V > 1 and logits.stride(1) != 1:
        raise ValueError("select_token: the vocabulary dimension must be unit-stride")
    row_stride = logits.stride(0) if B > 1 else max(V, logits.stride(0))
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=logits.device)
    if out_i32 is None:
        out_i32 = torch.empty(B, dtype=torch.int32, device=logits.device)
    for name, t, dt, n in (("out", out, torch.float32, B), ("out_i32", out_i32, torch.int32, B),
                           ("done", done, torch.int32, B), ("step_dev", step_dev, torch.int32, 1),
                           ("seed_dev", seed_dev, torch.int64, 1)):
        if t is not None and (not t.is_cuda or t.dtype != dt or t.numel() != n or not t.is_contiguous()):
            raise ValueError(f"select_token: {name} must be a contiguous device {dt} tensor of {n} element(s)")
    hs = 0
    if history is not None:
        if (not history.is_cuda or history.dtype != torch.int32 or history.dim() != 2 or history.shape[0] != B
                or history.stride(1) != 1):
            raise ValueError(f"select_token: history must be a device int32 [{B}, S] tensor with unit-stride rows")
        if step_dev is None:
            raise ValueError("select_token: history needs step_dev")
        # rows of S slots: a step at or past S is dropped by the kernel
        hs = history.shape[1]
        if B > 1 and history.stride(0) != hs:
            raise ValueError("select_token: history rows must be contiguous")
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    st = stream_ptr(logits.device) if stream is None else stream
    fn, filters = _nucleus_entry("mt_select_token", float(top_p), float(min_p))
    check(fn(
        logits.data_ptr(), B, V, row_stride, float(temperature), int(top_k),
        *((float(top_p), float(min_p)) if filters else ()), int(seed) & 0xFFFFFFFFFFFFFFFF,
        ptr(seed_dev), -1 if eos_id is None else int(eos_id), out.data_ptr(), out_i32.data_ptr(), ptr(done),
        ptr(history), hs, ptr(step_dev), st), "mt_select_token_p")
    return out, out_i32


def _spec_vec(who, name, t, n, dtype=None, optional=False):
    torch = _torch()
    dtype = torch.int32 if dtype is None else dtype
    if t is None and optional:
        return None
    if t is None or not t.is_cuda or t.dtype != dtype or t.numel() != n or not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be a contiguous device {dtype} tensor of {n} element(s)")
    return t.data_ptr()


def _spec_rows(who, name, t, B):
    """(S, row stride) of an int32 device [B, S] tensor with unit-stride rows."""
    torch = _torch()
    if (t is None or not t.is_cuda or t.dtype != torch.int32 or t.dim() != 2 or t.shape[0] != B
            or (t.shape[1] > 1 and t.stride(1) != 1)):
        raise ValueError(f"{who}: {name} must be a device int32 [{B}, S] tensor with unit-stride rows")
    return t.shape[1], (t.stride(0) if B > 1 else max(t.shape[1], t.stride(0)))


def spec_draft(tokens, held, k: int, max_ngram: int = 3, feed_f32=None, feed_i32=None, n_draft=None,
               stream: Optional[int] = None):
    """Prompt-lookup drafts (mt_spec_draft): tokens int32 [B, S] (row b: the prompt and everything
    emitted, held[b] tokens; read only), held int32 [B]. Returns (feed_f32, feed_i32, n_draft):
    the fp32 and int32 [B, k + 1] fed tokens (the last held token, then k drafts) and the int32
    [B] draft counts, allocated when not given. The rule is the header's."""
    torch = _torch()
    who = "spec_draft"
    if tokens is None or tokens.dim() != 2:
        raise ValueError(f"{who}: tokens must be a device int32 [B, S] tensor")
    B = tokens.shape[0]
    S, ts = _spec_rows(who, "tokens", tokens, B)
    n = B * (int(k) + 1)
    if feed_f32 is None:
        feed_f32 = torch.empty((B, int(k) + 1), dtype=torch.float32, device=tokens.device)
    if feed_i32 is None:
        feed_i32 = torch.empty((B, int(k) + 1), dtype=torch.int32, device=tokens.device)
    if n_draft is None:
        n_draft = torch.empty(B, dtype=torch.int32, device=tokens.device)
    st = stream_ptr(tokens.device) if stream is None else stream
    check(lib().mt_spec_draft(
        tokens.data_ptr(), B, S, ts, _spec_vec(who, "held", held, B), int(k), int(max_ngram),
        _spec_vec(who, "feed_f32", feed_f32, n, torch.float32), _spec_vec(who, "feed_i32", feed_i32, n),
        _spec_vec(who, "n_draft", n_draft, B), st), "mt_spec_draft")
    return feed_f32, feed_i32, n_draft


def spec_accept(logits, feed_i32, n_draft, limit, count, held, done, tokens, history, scratch=None,
                cache_len=None, drafted=None, accepted=None, steps=None, temperature: float = 0.0, top_k: int = 0,
                seed: int = 0, seed_dev=None, eos_id=None, stream: Optional[int] = None, top_p: float = 1.0,
                min_p: float = 0.0):
    """Verify the drafts of one speculative step and do its bookkeeping (mt_spec_accept_p): logits a
    3-D fp32 device view [B, k + 1, V] with unit-stride columns; feed_i32 / n_draft as spec_draft
    wrote them; limit, count, held, done (and the optional cache_len, drafted, accepted, steps)
    int32 [B]; tokens, history int32 [B, S] / [B, S']; scratch int32 [B, k + 1] (allocated when
    None; pass one inside a captured step). seed / seed_dev: the call's base seed (token number
    count[b] + i draws with base + count[b] + i); top_p / min_p: select_token's. Everything is
    updated in place; returns scratch, which then holds the k + 1 chosen ids of every row that was
    not done."""
    torch = _torch()
    who = "spec_accept"
    _check_dev(logits)
    if logits.dim() != 3 or logits.dtype != torch.float32:
        raise ValueError(f"{who} takes a 3-D float32 [B, k + 1, V] view, got {tuple(logits.shape)} {logits.dtype}")
    B, n, V = logits.shape
    if V > 1 and logits.stride(2) != 1:
        raise ValueError(f"{who}: the vocabulary dimension must be unit-stride")
    k = n - 1
    row_stride = logits.stride(1) if n > 1 else max(V, logits.stride(1))
    batch_stride = logits.stride(0) if B > 1 else max(k * row_stride + V, logits.stride(0))
    if scratch is None:
        scratch = torch.empty((B, n), dtype=torch.int32, device=logits.device)
    S, ts = _spec_rows(who, "tokens", tokens, B)
    hs, hstride = _spec_rows(who, "history", history, B)
    if B > 1 and hstride != hs:
        raise ValueError(f"{who}: history rows must be contiguous")
    v = lambda name, t, m=B, **kw: _spec_vec(who, name, t, m, **kw)  # noqa: E731
    st = stream_ptr(logits.device) if stream is None else stream
    fn, filters = _nucleus_entry("mt_spec_accept", float(top_p), float(min_p))
    check(fn(
        logits.data_ptr(), B, k, V, batch_stride, row_stride, v("feed_i32", feed_i32, B * n), v("n_draft", n_draft),
        float(temperature), int(top_k), *((float(top_p), float(min_p)) if filters else ()),
        int(seed) & 0xFFFFFFFFFFFFFFFF,
        v("seed_dev", seed_dev, 1, dtype=torch.int64, optional=True), -1 if eos_id is None else int(eos_id),
        v("limit", limit), v("count", count), v("held", held), v("cache_len", cache_len, optional=True),
        v("done", done), v("drafted", drafted, optional=True), v("accepted", accepted, optional=True),
        v("steps", steps, optional=True), tokens.data_ptr(), S, ts, history.data_ptr(), hs,
        v("scratch", scratch, B * n), st), "mt_spec_accept_p")
    return scratch


def rope(x, cos, sin, pos0=None, inverse: bool = False, out=None, x2=None, out2=None,
         stream: Optional[int] = None):
    """Rotary position embedding of the head rows of x [B,H,T,d] (mt_rope; fp32, any strides with
    unit-stride d) by the fp32 device tables cos / sin [n_pos, d/2], in the half-split convention.
    Token t of batch row b sits at min(max(pos0[b], 0) + t, n_pos - 1); pos0: a device int32 [B]
    (used as it is, read when the kernel runs), anything else is converted, None is 0.
    inverse: the transposed rotation (-sin). out: where the result goes (allocated dense when
    None; `out is x` rotates in place). x2 / out2: an optional second tensor [B,H2,T,d] (K beside
    Q) rotated in the same launch. Returns out, or (out, out2) with x2."""
    torch = _torch()
    _check_dev(x, cos, sin)
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError(f"rope takes a 4-D float32 [B,H,T,d] tensor, got {tuple(x.shape)} {x.dtype}")
    B, H, T, d = x.shape
    for t in (cos, sin):
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] * 2 != d or not t.is_contiguous():
            raise ValueError(f"rope: cos / sin must be dense float32 [n_pos, {d // 2}] tables, got {tuple(t.shape)}")
    if cos.shape != sin.shape:
        raise ValueError("rope: the cos and sin tables differ in shape")
    if out is None:
        out = torch.empty((B, H, T, d), dtype=torch.float32, device=x.device)
    if tuple(out.shape) != (B, H, T, d) or out.dtype != torch.float32 or not out.is_cuda:
        raise ValueError(f"rope: out must be a device float32 {[B, H, T, d]} tensor")
    H2 = 0
    if x2 is not None:
        _check_dev(x2)
        if x2.dim() != 4 or x2.dtype != torch.float32 or (x2.shape[0], x2.shape[2], x2.shape[3]) != (B, T, d):
            raise ValueError(f"rope: x2 must be a float32 [{B}, H2, {T}, {d}] tensor, got {tuple(x2.shape)}")
        H2 = x2.shape[1]
        if out2 is None:
            out2 = torch.empty((B, H2, T, d), dtype=torch.float32, device=x.device)
        if tuple(out2.shape) != tuple(x2.shape) or out2.dtype != torch.float32 or not out2.is_cuda:
            raise ValueError(f"rope: out2 must be a device float32 {[B, H2, T, d]} tensor")
    p = _kv_arg(pos0, B, x.device)
    st = stream_ptr(x.device) if stream is None else stream
    check(lib().mt_rope(
        MT_F32, int(bool(inverse)), x.data_ptr(), out.data_ptr(), H, strides3(x), strides3(out),
        None if x2 is None else x2.data_ptr(), None if x2 is None else out2.data_ptr(), H2,
        None if x2 is None else strides3(x2), None if x2 is None else strides3(out2),
        B, T, d, cos.data_ptr(), sin.data_ptr(), cos.shape[0], None if p is None else p.data_ptr(), st),
        "mt_rope")
    return out if x2 is None else (out, out2)


def scratch_bytes() -> int:
    """Device bytes the library's stream scratch holds between calls (mt_scratch_bytes)."""
    return int(lib().mt_scratch_bytes())


def scratch_release() -> None:
    """Free the library's stream scratch that no captured graph holds (mt_scratch_release)."""
    check(lib().mt_scratch_release(), "mt_scratch_release")


def matmul_plan(backend: int, batch: int, M: int, N: int, K: int, a_strides, b_strides, c_strides,
                a_ptr: int = 0, b_ptr: int = 0, c_ptr: int = 0):
    """(kernel, ak, bk, vec, S, ks) of mt_matmul_f32 for this problem under GEMM backend `backend`
    (mt_matmul_f32_plan: kernel 0 rocBLAS, 1 rocBLAS on own K slices, 2 the fp32-MFMA kernel,
    3 / 4 the X3 GEMM on 64x64 / 128x128 tiles). Strides are (batch, row, col) triples in
    elements; the pointers count for their alignment only. No device call."""
    out = (ctypes.c_int32 * 5)()
    s3 = lambda s: (ctypes.c_int64 * 3)(*[int(x) for x in s])  # noqa: E731
    kern = lib().mt_matmul_f32_plan(backend, batch, M, N, K, s3(a_strides), s3(b_strides), s3(c_strides),
                                    a_ptr or None, b_ptr or None, c_ptr or None, out)
    if kern < 0:
        raise ValueError(lib().mt_last_error().decode(errors="replace"))
    return (kern, *out)


def exported_symbols() -> Sequence[str]:
    return tuple(_PROTOS)


def adam_step(params, grads, exp_avg, exp_avg_sq, numels, beta1, beta2, eps, step_size,
              step_size_ptr: Optional[int] = None) -> None:
    """One multi-tensor Adam launch (mt_adam_step) over dense fp32 device buffers given as
    raw pointers, in place, on the current stream. step_size_ptr: read the step size from
    that device fp32 instead (mt_adam_step_dstep, a graph-captured step)."""
    n = len(params)
    arr = ctypes.c_void_p * max(1, n)
    ptrs = (n, arr(*params), arr(*grads), arr(*exp_avg), arr(*exp_avg_sq), (ctypes.c_int64 * max(1, n))(*numels),
            beta1, beta2, eps)
    if step_size_ptr is None:
        check(lib().mt_adam_step(*ptrs, step_size, stream_ptr()), "mt_adam_step")
    else:
        check(lib().mt_adam_step_dstep(*ptrs, step_size_ptr, stream_ptr()), "mt_adam_step_dstep")
