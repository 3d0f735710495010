"""ctypes side of vox_debug_xf_op (include/voxtral_hip.h): the descriptor, the buffer block and one call (tests/test_gpu_xf_ops.py, tests/test_abi_cpu.py)."""
import ctypes as C

import numpy as np

EPI_STORE, EPI_ROPE_KV, EPI_SWIGLU_XF, EPI_RESID_XF = 0, 1, 2, 3
KV_CONTIG, KV_SLOTS, KV_PAGED, KV_PAGED_RING = 0, 1, 2, 3
MODE_STEP, MODE_ROWS, MODE_WIDE_ROWS = 0, 1, 2
_I = ("mode", "groups", "M", "epi", "n_part")
_J = ("hd", "n_q", "n_kv", "kv_form", "kv_bf16", "kv_slices", "kv_rows", "rope_rows", "rope_mask", "rope_seq_rows", "xf_in_gs", "xf_out_gs", "ssq_part_gs", "ssq_out_gs",
      "plan_ntw", "plan_ks", "plan_steps", "plan_straight", "fused_rope", "pos_off")
BUF_NAMES = ("x", "ssq_part", "bias", "resid", "xf_w", "xf_w2", "rope_cos", "rope_sin", "pos", "kv_row", "kv_pos", "rope_member", "out", "kc", "vc", "xf_out", "ssq_out")


class XfOpDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in _I] + [("norm_eps", C.c_float)] + [(n, C.c_int32) for n in _J] + [("reserved", C.c_int32 * 2)]


class XfOpBufs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in BUF_NAMES]


def call(pkg, ctx_h, w_h, desc, **arrays):
    """One vox_debug_xf_op call; arrays: numpy arrays (kept alive here) by buffer name, None = null.  Returns the status code."""
    b = XfOpBufs()
    for n, a in arrays.items():
        assert n in BUF_NAMES, n
        if a is not None:
            assert a.flags["C_CONTIGUOUS"]
            setattr(b, n, a.ctypes.data_as(C.c_void_p))
    return pkg.lib().vox_debug_xf_op(ctx_h, w_h, C.byref(desc), C.byref(b))


def sentinel32(shape):
    """f32 buffer of one NaN bit pattern no kernel produces."""
    return np.full(shape, 0x7FC0BEEF, np.uint32).view(np.float32)


def is_sentinel32(a):
    return np.ascontiguousarray(a).view(np.uint32) == 0x7FC0BEEF


SENT16 = 0xBEEF
