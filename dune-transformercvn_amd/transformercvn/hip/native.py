"""What every caller of libtcvn_hip.so shares: ctypes arguments from tensors and streams, and the GPU-only guard."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch


def ptr(t: Optional[torch.Tensor]) -> C.c_void_p:
    """The tensor's address; NULL for None."""
    return C.c_void_p(0 if t is None else t.data_ptr())


def ptr_or_null(t: Optional[torch.Tensor]) -> C.c_void_p:
    """The tensor's address; NULL for None and for a tensor without elements."""
    return C.c_void_p(0 if t is None or t.numel() == 0 else t.data_ptr())


def stream_ptr(device=None) -> C.c_void_p:
    """The current stream of `device` (None: of the current device)."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def gpu_only(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise RuntimeError(f"transformercvn (MI355X build): {what} runs on the GPU only; there is no CPU fallback")
