"""What the two mesh evaluators (gs2m_dtu_eval.py, gs2m_tnt_eval.py) share on the host side: device and tensor plumbing for
the fp64 point kernels of csrc/mesh_eval.hip and the compaction."""
import ctypes as C

import torch

import gs2m_native as N

ptr = N.ptr


def device(dev):
    return torch.device(dev if dev is not None else "cuda")


def points(a, dev):
    """(n, 3) fp64 contiguous tensor on `dev` (numpy or torch input; a tensor that already is one comes back as it is)."""
    t = torch.as_tensor(a)
    return t.to(device=dev, dtype=torch.float64).reshape(-1, 3).contiguous()


def workspace(nbytes, dev):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)


def compact(p, flags, bit, dev):
    """The points whose flag byte has `bit` set, in index order.  -> a view of the first rows of a buffer of len(p) rows:
    clone it to let the buffer go."""
    wb = C.c_longlong()
    N.check(N.lib().gs2m_eval_scan_workspace_bytes(len(p), C.byref(wb)), "gs2m_eval_scan_workspace_bytes")
    out = torch.empty_like(p)
    cnt = C.c_longlong()
    ws = workspace(wb.value, dev)
    N.launch("gs2m_eval_compact", dev, len(p), ptr(p), ptr(flags), int(bit), ptr(ws), ptr(out), C.byref(cnt))
    return out[:cnt.value]
