"""Thin tensor-level wrappers over the C ABI (one function per entry point).

All tensors must live on the HIP device, fp32 / int32 / int64 as documented in
include/gamer_hip.h.  Kernels are enqueued on torch's current stream.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import os

import torch

from . import _lib
from ._lib import GemmBf16Desc, GemmDesc, call, ptr, stream_ptr


def _sfx(t: torch.Tensor) -> str:
    """Entry-point suffix for the activation dtype of ``t``: fp32 -> "", bf16 -> "_bf16" (the AMP variant)."""
    if t.dtype == torch.float32:
        return ""
    if t.dtype == torch.bfloat16:
        return "_bf16"
    raise RuntimeError(f"activations must be float32 or bfloat16, got {t.dtype}")


def _chk(t: torch.Tensor, dtype, name: str):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be on the HIP device (gamer_amd has no CPU path)")
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must be {dtype}, got {t.dtype}")


# ----------------------------------------------------------------------------------------------
def reload_env():
    """The library caches its GAMER_* kernel switches (one read per process): call this after changing os.environ in-process."""
    call("gamer_reload_env")


class env_switches:
    """`with env_switches(GAMER_GEMM_AS=0): ...` - set GAMER_* kernel switches for a block inside a running process (tests, A/B
    tools) and have the library read them again on entry and exit."""

    def __init__(self, **kw):
        self.kw = {k: str(v) for k, v in kw.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)
        reload_env()
        return self

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        reload_env()


def router_fwd(ids, attn_mask, actions, behavior_lut, num_positions, pad_id, eos_id, out: dict):
    B, S = ids.shape
    _chk(ids, torch.int64, "input_ids")
    call("gamer_router_fwd", ptr(ids), ptr(attn_mask), ptr(actions), ptr(behavior_lut), behavior_lut.numel(),
         B, S, num_positions, pad_id, eos_id,
         ptr(out["expert"]), ptr(out["beh_idx"]), ptr(out["act_idx"]),
         ptr(out["kl_self"]), ptr(out["kl_cross"]), ptr(out["ql_cross"]),
         ptr(out["empty_self"]), ptr(out["empty_cross"]),
         ptr(out["tile_empty_self"]), ptr(out["tile_empty_cross"]), ptr(out["bad_token"]), stream_ptr())


def alloc_router_outputs(B, S, device):
    n_tiles = (S + 31) // 32
    i32 = dict(dtype=torch.int32, device=device)
    out = {k: torch.empty(B, S, **i32) for k in
           ("expert", "beh_idx", "act_idx", "kl_self", "kl_cross", "ql_cross", "empty_self", "empty_cross")}
    out["tile_empty_self"] = torch.empty(B, n_tiles, **i32)
    out["tile_empty_cross"] = torch.empty(B, n_tiles, **i32)
    out["bad_token"] = torch.zeros(1, **i32)
    return out


def alloc_session_outputs(B, S, device):
    i32 = dict(dtype=torch.int32, device=device)
    return {"span_self": torch.empty(B, S, 4, **i32), "span_cross": torch.empty(B, S, 4, **i32),
            "pos_ids": torch.empty(B, S, **i32), "violations": torch.zeros(1, **i32)}


def session_spans(session_ids, extended_session_ids, attn_mask, num_positions, n_rope_positions, router: dict,
                  out: dict):
    """Qwen3SessionMulti masks as per-query key spans (gamer_session_spans).  Run after router_fwd: overwrites the
    router's empty_* / tile_empty_* with the session masks' empty rows."""
    B, S = session_ids.shape
    _chk(session_ids, torch.int64, "session_ids")
    if extended_session_ids is not None:
        _chk(extended_session_ids, torch.int64, "extended_session_ids")
    call("gamer_session_spans", ptr(session_ids), ptr(extended_session_ids), ptr(attn_mask), ptr(router["kl_cross"]),
         ptr(router["ql_cross"]), B, S, num_positions, n_rope_positions, ptr(out["span_self"]),
         ptr(out["span_cross"]), ptr(out["pos_ids"]), ptr(router["empty_self"]), ptr(router["empty_cross"]),
         ptr(router["tile_empty_self"]), ptr(router["tile_empty_cross"]), ptr(out["violations"]), stream_ptr())


def causal_prep(attn_mask, B, S, kl_self, empty_self, tile_empty_self, pos_ids=None, next_pos=None):
    """Causal + key-padding mask of the Qwen3 baseline and (optionally) generate()'s per-row RoPE positions
    (gamer_causal_prep).  attn_mask: int64 [B,S] or None."""
    if attn_mask is not None:
        _chk(attn_mask, torch.int64, "attention_mask")
    call("gamer_causal_prep", ptr(attn_mask), B, S, ptr(kl_self), ptr(empty_self), ptr(tile_empty_self), ptr(pos_ids),
         ptr(next_pos), stream_ptr())


def moe_router_prep(ids, attn_mask, behavior_lut, position_table, num_positions, n_items, use_behavior_token, pad_id,
                    eos_id, out: dict, pos_ids=None, next_pos=None):
    """Qwen3Moe's router outputs and causal + key-padding mask in one launch (gamer_moe_router_prep).  ``out``: expert,
    beh_idx, kl_self, empty_self, tile_empty_self, bad_token (incremented, not cleared).  ``position_table``: int32
    [num_positions] on the device or None (position p -> expert p + 1).  ``pos_ids`` / ``next_pos``: generate()'s per-row
    RoPE positions of a left-padded prompt (see causal_prep), or None."""
    B, S = ids.shape
    _chk(ids, torch.int64, "input_ids")
    if attn_mask is not None:
        _chk(attn_mask, torch.int64, "attention_mask")
    if position_table is not None:
        _chk(position_table, torch.int32, "position_table")
        if position_table.numel() != num_positions:
            raise ValueError(f"position_table has {position_table.numel()} entries, num_positions is {num_positions}")
    call("gamer_moe_router_prep", ptr(ids), ptr(attn_mask), ptr(behavior_lut),
         behavior_lut.numel() if behavior_lut is not None else 0, ptr(position_table), B, S, num_positions, n_items,
         1 if use_behavior_token else 0, pad_id, eos_id, ptr(out["expert"]), ptr(out["beh_idx"]), ptr(out["kl_self"]),
         ptr(out["empty_self"]), ptr(out["tile_empty_self"]), ptr(pos_ids), ptr(next_pos), ptr(out["bad_token"]),
         stream_ptr())


MAX_EXPERT_GROUPS = 64          # gamer_expert_lists: row groups at most


def moe_action_router_prep(ids, attn_mask, behavior_lut, position_table, num_positions, n_items, use_behavior_token, pad_id,
                           eos_id, num_position_experts, num_ffn_experts, out: dict, pos_ids=None, next_pos=None,
                           act_zero_col=None):
    """Qwen3MoeAction's router outputs and causal + key-padding mask in one launch (gamer_moe_action_router_prep): the
    arguments and outputs of ``moe_router_prep``, plus ``out["act_idx"]`` and ``out["expert"]`` = the FFN's index
    max(0, num_position_experts * (act_idx - 1) + position expert) among ``num_ffn_experts`` experts.  ``act_zero_col``: a
    column whose action index is forced to 0 (a generation's re-run), or None."""
    B, S = ids.shape
    _chk(ids, torch.int64, "input_ids")
    if attn_mask is not None:
        _chk(attn_mask, torch.int64, "attention_mask")
    if position_table is not None:
        _chk(position_table, torch.int32, "position_table")
        if position_table.numel() != num_positions:
            raise ValueError(f"position_table has {position_table.numel()} entries, num_positions is {num_positions}")
    if not 0 < num_ffn_experts <= MAX_EXPERT_GROUPS:
        raise ValueError(f"num_ffn_experts = {num_ffn_experts}: the expert lists (gamer_expert_lists) hold at most "
                         f"{MAX_EXPERT_GROUPS} groups")
    call("gamer_moe_action_router_prep", ptr(ids), ptr(attn_mask), ptr(behavior_lut),
         behavior_lut.numel() if behavior_lut is not None else 0, ptr(position_table), B, S, num_positions, n_items,
         1 if use_behavior_token else 0, pad_id, eos_id, num_position_experts, -1 if act_zero_col is None else int(act_zero_col),
         ptr(out["expert"]), ptr(out["beh_idx"]), ptr(out["act_idx"]), ptr(out["kl_self"]), ptr(out["empty_self"]),
         ptr(out["tile_empty_self"]), ptr(pos_ids), ptr(next_pos), ptr(out["bad_token"]), stream_ptr())


def session_prep(session_ids, extended_session_ids, attn_mask, num_positions, n_rope_positions, out: dict):
    """Qwen3Session's self mask as per-query key spans plus its RoPE positions, without a router (gamer_session_prep).
    ``out``: kl_self, span_self, pos_ids, empty_self, tile_empty_self, violations (incremented, not cleared)."""
    B, S = session_ids.shape
    _chk(session_ids, torch.int64, "session_ids")
    if extended_session_ids is not None:
        _chk(extended_session_ids, torch.int64, "extended_session_ids")
    if attn_mask is not None:
        _chk(attn_mask, torch.int64, "attention_mask")
    call("gamer_session_prep", ptr(session_ids), ptr(extended_session_ids), ptr(attn_mask), B, S, num_positions,
         n_rope_positions, ptr(out["kl_self"]), ptr(out["span_self"]), ptr(out["pos_ids"]), ptr(out["empty_self"]),
         ptr(out["tile_empty_self"]), ptr(out["violations"]), stream_ptr())


def session_moe_prep(ids, attn_mask, session_ids, extended_session_ids, behavior_lut, position_table, num_positions,
                     n_items, use_behavior_token, pad_id, eos_id, n_rope_positions, out: dict):
    """Qwen3SessionMoe's one prep launch (gamer_session_moe_prep): the router outputs of ``moe_router_prep`` (``out``:
    expert, beh_idx, bad_token) and the mask outputs of ``session_prep`` (``out``: kl_self, span_self, pos_ids, empty_self,
    tile_empty_self, violations); bad_token and violations are incremented, not cleared."""
    B, S = ids.shape
    _chk(ids, torch.int64, "input_ids")
    _chk(session_ids, torch.int64, "session_ids")
    if tuple(session_ids.shape) != (B, S):
        raise ValueError(f"session_ids has shape {tuple(session_ids.shape)}, input_ids {(B, S)}")
    if extended_session_ids is not None:
        _chk(extended_session_ids, torch.int64, "extended_session_ids")
        if tuple(extended_session_ids.shape) != (B, S):
            raise ValueError(f"extended_session_ids has shape {tuple(extended_session_ids.shape)}, input_ids {(B, S)}")
    if attn_mask is not None:
        _chk(attn_mask, torch.int64, "attention_mask")
    if position_table is not None:
        _chk(position_table, torch.int32, "position_table")
        if position_table.numel() != num_positions:
            raise ValueError(f"position_table has {position_table.numel()} entries, num_positions is {num_positions}")
    call("gamer_session_moe_prep", ptr(ids), ptr(attn_mask), ptr(session_ids), ptr(extended_session_ids), ptr(behavior_lut),
         behavior_lut.numel() if behavior_lut is not None else 0, ptr(position_table), B, S, num_positions, n_items,
         1 if use_behavior_token else 0, pad_id, eos_id, n_rope_positions, ptr(out["expert"]), ptr(out["beh_idx"]),
         ptr(out["bad_token"]), ptr(out["kl_self"]), ptr(out["span_self"]), ptr(out["pos_ids"]), ptr(out["empty_self"]),
         ptr(out["tile_empty_self"]), ptr(out["violations"]), stream_ptr())


def router_position_table(expert, table):
    """expert[i] <- table[expert[i]] in place (gamer_router_position_table; int32 tensors on the device)."""
    _chk(expert, torch.int32, "expert")
    _chk(table, torch.int32, "table")
    call("gamer_router_position_table", ptr(expert), expert.numel(), ptr(table), table.numel(), stream_ptr())


def expert_lists(expert, num_experts, perm, slot, offsets, work):
    B, S = expert.shape
    call("gamer_expert_lists", ptr(expert), B, S, num_experts, ptr(perm), ptr(slot), ptr(offsets), ptr(work),
         stream_ptr())


def embedding_fwd(ids, W, x):
    T = ids.numel()
    V, H = W.shape
    call("gamer_embedding_fwd", ptr(ids), ptr(W), V, T, H, ptr(x), stream_ptr())


def embedding_bwd(ids, dx, pad_id, dW):
    T = ids.numel()
    V, H = dW.shape
    call("gamer_embedding_bwd", ptr(ids), ptr(dx), V, T, H, pad_id, ptr(dW), stream_ptr())


_EMB_WS = {}


def embedding_bwd_ordered(ids, dx, pad_id, dW):
    """dW[id] += dx rows, without float atomics: the same bits on every run (gamer_embedding_bwd_ordered)."""
    T = ids.numel()
    V, H = dW.shape
    need = int(_lib.load().gamer_embedding_bwd_ordered_ws_bytes(V, T, H))
    ws = _EMB_WS.get(dx.device)
    if ws is None or ws.numel() < need:
        _EMB_WS[dx.device] = None
        ws = _EMB_WS[dx.device] = torch.empty(need, dtype=torch.uint8, device=dx.device)
    call("gamer_embedding_bwd_ordered", ptr(ids), ptr(dx), V, T, H, pad_id, ptr(dW), ptr(ws), ws.numel(), stream_ptr())


def rmsnorm_fwd(x, w, eps, y, ldy=None, dst_rows=None):
    T, H = x.shape
    ld = ldy if ldy else y.stride(0)
    _arm_sink((y, (1, 0, T, ld, ld), False))       # (the consumer GEMM reads rows of ld columns: rowtable_fwd adds the rest)
    call("gamer_rmsnorm_fwd" + _sfx(y), ptr(x), ptr(w), T, H, eps, ptr(dst_rows), ptr(y), ld, stream_ptr())


def rmsnorm_bwd(x, w, dy, lddy, eps, dx, dw_partial, accumulate_dx=True, dy_rows=None, mask_out=None, mask_rows=None,
                p=0.0, seed=0):
    """mask_out: also write dropout_mask(seed) * dx (the input gradient of the next residual branch), rows scattered
    through mask_rows when given - the second pass gamer_residual_dropout_bwd would make over dx."""
    T, H = x.shape
    if mask_out is not None:
        _arm_sink((mask_out, (1, 0, T, H, H), False))
    call("gamer_rmsnorm_bwd" + _sfx(dy), ptr(x), ptr(w), ptr(dy), lddy, ptr(dy_rows), T, H, eps, 1 if accumulate_dx else 0,
         ptr(dx), ptr(dw_partial), dw_partial.shape[0], ptr(mask_out), ptr(mask_rows), p, seed, stream_ptr())


def colsum_reduce(partial, out, accumulate=False):
    rows, cols = partial.shape
    call("gamer_colsum_reduce", ptr(partial), rows, cols, 1 if accumulate else 0, ptr(out), stream_ptr())


def colsum_reduce_batched(partials, n, outs_table, accumulate=False):
    """partials [>= n, rows, cols] (contiguous); outs_table: int64 device tensor of n output addresses."""
    _, rows, cols = partials.shape
    call("gamer_colsum_reduce_batched", ptr(partials), rows * cols, rows, cols, n, ptr(outs_table), 1 if accumulate else 0,
         stream_ptr())


def rowtable_fwd(table, idx, y, ldy, col0, dst_rows=None):
    T = idx.numel()
    E = table.shape[1]
    _arm_sink((y, (1, 0, T, ldy, ldy), "only"))    # joins the slot the RMSNorm that wrote the other columns opened, if any
    call("gamer_rowtable_fwd" + _sfx(y), ptr(table), ptr(idx), ptr(dst_rows), T, E, ptr(y), ldy, col0, stream_ptr())


def rowtable_bwd(dy, lddy, col0, idx, dtable, dy_rows=None, partial=None):
    """partial: fp32 scratch (>= rows * E floats): the ordered form (no float atomics, same bits on every run)."""
    T = idx.numel()
    rows, E = dtable.shape
    call("gamer_rowtable_bwd" + _sfx(dy), ptr(dy), lddy, col0, ptr(idx), ptr(dy_rows), T, E, rows, ptr(dtable), ptr(partial),
         partial.numel() if partial is not None else 0, stream_ptr())


# fp32 matmul form in effect: 0 = v_mfma_f32_32x32x2_f32, 6 / 9 = gamer_gemm_f32_split (exact three-way bf16 cut of both
# operands, 6 or 9 piece products on the bf16 pipe), 3 = its two-way fp16 form (per-tensor power-of-two scales from
# gamer_absmax_f32, 3 piece products).  Default 0; an Engine / DecodeSession with another form scopes its
# own calls with `with ops.f32_matmul(form):`, which restores the previous value on exit - two engines with different
# forms, tools and tests in one process do not leak their setting into each other.
F32_MATMUL_TERMS = 0
MATMUL_MODES = {"f32": 0, "split3": 3, "split6": 6, "split9": 9}
# Pre-cut weights of the split forms: (address of the fp32 flat parameter buffer, its bytes, address of the three bf16 planes,
# plane stride in elements) or None.  Set - scoped, like the matmul form - by the engine that owns the buffers; gemm() hands a
# B operand that lies inside the flat buffer to gamer_gemm_f32_split together with its planes.
WEIGHT_PLANES = None


class f32_matmul:
    """Context manager: fp32 GEMMs issued inside the block use `mode` ("f32" | "split6" | "split9" or 0 / 6 / 9)."""

    def __init__(self, mode, planes=None):
        self.mode, self.planes = mode, planes

    def __enter__(self):
        global WEIGHT_PLANES
        self.prev = set_f32_matmul(self.mode)
        self.prev_planes = WEIGHT_PLANES
        WEIGHT_PLANES = self.planes
        return self

    def __exit__(self, *exc):
        global WEIGHT_PLANES
        set_f32_matmul(self.prev)
        WEIGHT_PLANES = self.prev_planes
        return False


def scoped_f32_matmul(get_mode, get_planes=None):
    """Decorator form of f32_matmul: `get_mode(*args)` names the form for the duration of the call, `get_planes(*args)`
    (optional) the pre-cut weight planes (WEIGHT_PLANES)."""
    import functools

    def deco(fn):
        @functools.wraps(fn)
        def wrapper(*args, **kwargs):
            with f32_matmul(get_mode(*args), get_planes(*args) if get_planes is not None else None):
                return fn(*args, **kwargs)
        return wrapper
    return deco


# split3: one device word per operand tensor for the bits of its largest magnitude.  Slots come from a ring that is zeroed as a
# whole when it wraps (stream-ordered: every GEMM that read an old slot was enqueued before the memset).
_AMAX_RING = {}
_AMAX_SLOTS = 1024
AMAX_WORDS = 256            # GAMER_AMAX_WORDS: one maximum = 16 words 64 bytes apart (producers spread their atomics over them)
# Optional reuse of a maximum for a tensor that is read by several GEMMs while it does not change (x by forward and weight
# gradient, dy by weight and input gradient, a weight by every GEMM of a step): inside `with cache:` (an amax_reuse) a slot is
# keyed by (address, extent) and measured once for tensors the OWNER declared unchanging - `stable(...)` tensors / address
# ranges until the next `reset()`, `hold(...)` tensors for the duration of a with-block.  Everything else is measured per GEMM.
_AMAX_REUSE = None


class amax_reuse:
    def __init__(self, everything=False):
        self.slots, self.pending, self.pools, self.used = {}, {}, [], 0
        self.stable_ptrs, self.stable_ranges, self.held = set(), [], {}
        # dense tensors inside the FIRST stable range (the parameter buffer) that GEMMs asked for: measured together by one
        # launch at the start of the next pass (gamer_absmax_multi_f32) instead of one launch each
        self._wkeys, self._wtable, self._wtable_n = [], None, 0
        # (a buffer of the parameter buffer's size, or None): the fp16 pieces of those tensors packed at their values' offsets,
        # rebuilt by the same pass-start launch pair; a GEMM whose B operand is exactly one of them reads them instead of cutting
        self.planes, self._plane_keys = None, set()
        # (a second buffer of the same size, or None): the packed pieces of the TRANSPOSES of registered matrices at their values'
        # offsets (register_transposed: the layers with 256 output features and a long contraction - their forward runs on the
        # output-stationary kernel, which wants W^T [K][256]); rebuilt from `planes` right after them
        self.planes_t, self._tkeys, self._ttable, self._tplane_keys = None, [], None, set()
        self.everything = everything          # tools: every tensor counts as unchanging (kernel timing)

    def __enter__(self):
        global _AMAX_REUSE
        self.prev, _AMAX_REUSE = _AMAX_REUSE, self
        return self

    def __exit__(self, *exc):
        global _AMAX_REUSE
        _AMAX_REUSE = self.prev
        return False

    def stable(self, *tensors):
        self.stable_ptrs.update(t.data_ptr() for t in tensors if t is not None)

    def stable_range(self, base, nbytes):
        self.stable_ranges.append((int(base), int(nbytes)))

    def reset(self):
        """Start of a forward pass: every cached maximum is dropped, the slot words are zeroed (one memset per pool)."""
        self.slots.clear()
        self.pending.clear()
        self.held.clear()
        self.stable_ptrs.clear()        # (the owner declares its unchanging tensors again: addresses of a freed workspace may be reused)
        for pool in self.pools:
            pool.zero_()
        self.used = 0
        if self._wkeys and self.stable_ranges and len(self._wkeys) <= 1024:
            base = self.stable_ranges[0][0]
            dev = self._wdev
            if self._wtable is None or self._wtable_n != len(self._wkeys):
                tab = [v for (p_, n_) in self._wkeys for v in ((p_ - base) // 4, n_)]
                self._wtable = torch.tensor(tab, dtype=torch.int64, device=dev)
                self._wtable_n = len(self._wkeys)
            first = self._new_slot(dev)
            for _ in range(len(self._wkeys) - 1):
                self._new_slot(dev)                 # (consecutive: a fresh pool holds 1024 slots)
            call("gamer_absmax_multi_f32", base, self._wtable.data_ptr(), len(self._wkeys), first, stream_ptr())
            for e, (p_, n_) in enumerate(self._wkeys):
                self.slots[(p_, "dense", n_)] = first + 4 * AMAX_WORDS * e
            self._plane_keys = set()
            if self.planes is not None:
                call("gamer_split2h_planes_multi", base, self._wtable.data_ptr(), len(self._wkeys), first, self.planes.data_ptr(),
                     stream_ptr())
                self._plane_keys = {(p_, "dense", n_) for (p_, n_) in self._wkeys}
                self._tplane_keys = set()
                if self.planes_t is not None and self._tkeys:
                    # every registered matrix whose tensor has pieces in this pass: one launch transposes them all
                    live = [(p_, b_, r_, c_) for (p_, b_, r_, c_) in self._tkeys if (p_, "dense", b_ * r_ * c_) in self._plane_keys]
                    if live:
                        if self._ttable is None or self._ttable[0] != live:
                            tab = [v for (p_, b_, r_, c_) in live for i in range(b_) for v in ((p_ - base) // 4 + i * r_ * c_, r_, c_)]
                            self._ttable = (live, torch.tensor(tab, dtype=torch.int64, device=dev), len(tab) // 3)
                        call("gamer_split2h_transpose_multi", self.planes.data_ptr(), self._ttable[1].data_ptr(), self._ttable[2],
                             self.planes_t.data_ptr(), stream_ptr())
                        self._tplane_keys = {(p_, "dense", b_ * r_ * c_) for (p_, b_, r_, c_) in live}

    def register(self, *tensors):
        """Dense parameter tensors (inside the first stable range) that GEMMs only ever read VIEWS of (the injecting layers'
        gate|up weight: its 256 hidden columns): measured and cut with the others from the next pass on (plane_parent)."""
        if not self.stable_ranges:
            return
        b0, n0 = self.stable_ranges[0]
        for t in tensors:
            p, n = t.data_ptr(), t.numel()
            if (b0 <= p and p + 4 * n <= b0 + n0 and n % 4 == 0 and t.is_contiguous() and
                    not any(p_ < p + 4 * n and p < p_ + 4 * n_ for (p_, n_) in self._wkeys)):
                self._wkeys.append((p, n))
                self._wdev = t.device

    def reserve(self, n):
        """Make sure `n` more slots exist without another pool allocation (a pool is zero-filled when it is allocated: a
        hipGraph capture must not contain that fill - replayed, it would wipe the maxima of everything measured before)."""
        while len(self.pools) * 1024 - self.used < n and self.pools:
            self.pools.append(torch.zeros(1024 * AMAX_WORDS, dtype=torch.int32, device=self.pools[0].device))

    def register_transposed(self, t, batch, rows, cols):
        """The dense parameter tensor `t` = `batch` row-major [rows][cols] matrices: from the next pass on the pieces of their
        transposes are kept beside the pieces of `t` (planes_t; see __init__)."""
        if self.planes_t is None or not t.is_contiguous() or t.numel() != batch * rows * cols or rows % 4 or cols % 4:
            return
        key = (t.data_ptr(), int(batch), int(rows), int(cols))
        if key not in self._tkeys:
            self._tkeys.append(key)
            self.register(t)

    def plane_parent(self, p, geom):
        """Slot of the maximum of the dense parameter tensor with piece planes that contains the operand view (p, geom) - or None
        (also when the view IS such a tensor: the exact-key path handles that)."""
        key = self._key(p, geom)
        if key in self._plane_keys or len(key) == 3:
            return None
        batch, stride, rows, cols, ld = geom
        end = p + 4 * ((batch - 1) * stride + (rows - 1) * ld + cols)
        for (p_, kind, n_) in self._plane_keys:
            if p_ <= p and end <= p_ + 4 * n_:
                return self.slots.get((p_, kind, n_))
        return None

    def hold(self, *tensors):
        cache = self

        class _Hold:
            def __enter__(self_h):
                for t in tensors:
                    cache.held[t.data_ptr()] = cache.held.get(t.data_ptr(), 0) + 1

            def __exit__(self_h, *exc):
                for t in tensors:
                    p = t.data_ptr()
                    cache.held[p] -= 1
                    if cache.held[p] == 0:
                        del cache.held[p]
                        for k in [k for k in cache.slots if k[0] == p]:
                            del cache.slots[k]
                return False
        return _Hold()

    def _cached(self, p):
        if self.everything or p in self.stable_ptrs or p in self.held:
            return True
        return any(b <= p < b + n for b, n in self.stable_ranges)

    @staticmethod
    def _key(p, geom):
        batch, stride, rows, cols, ld = geom
        if ld == cols and (batch == 1 or stride == rows * ld):
            return (p, "dense", batch * rows * cols)
        return (p,) + tuple(geom)

    def _new_slot(self, device):
        i, j = divmod(self.used, 1024)
        if i == len(self.pools):
            self.pools.append(torch.zeros(1024 * AMAX_WORDS, dtype=torch.int32, device=device))
        self.used += 1
        return self.pools[i].data_ptr() + 4 * AMAX_WORDS * j

    def preset(self, x, geom, accumulate=False):
        """A slot the PRODUCER of x is about to fill (gamer_amax_sink): the next GEMM that reads x with this extent takes
        it instead of measuring x.  accumulate: a second producer writing other columns of the same tensor."""
        key = self._key(x.data_ptr(), geom)
        if accumulate and key in self.pending:
            return self.pending[key]
        if accumulate == "only":                    # a later producer of a tensor whose first producer did not open a slot
            return None
        self.slots.pop(key, None)
        ptr_ = self.pending[key] = self._new_slot(x.device)
        return ptr_

    def peek(self, x, geom):
        """The slot `slot(x, geom)` would return without measuring - its producer's, or a cached one - or None; nothing is consumed
        (a generation's prompt pass notes the maxima of the keys / values it caches before the layer's attention takes them)."""
        key = self._key(x.data_ptr(), geom)
        return self.pending.get(key) or self.slots.get(key)

    def slot(self, x, geom):
        p = x.data_ptr()
        key = self._key(p, geom)
        keep = self._cached(p)
        if key in self.pending:                     # written by its producer together with the tensor
            ptr_ = self.pending.pop(key)
            if keep:
                self.slots[key] = ptr_
            return ptr_
        if keep and key in self.slots:
            return self.slots[key]
        ptr_ = self._new_slot(x.device)
        call("gamer_absmax_f32", ptr(x), *geom, ptr_, stream_ptr())
        if keep:
            self.slots[key] = ptr_
            if (len(key) == 3 and self.stable_ranges and key[2] % 4 == 0 and
                    self.stable_ranges[0][0] <= p < self.stable_ranges[0][0] + self.stable_ranges[0][1] and
                    not any(p_ < p + 4 * key[2] and p < p_ + 4 * n_ for (p_, n_) in self._wkeys)):
                # a parameter tensor: part of the one-launch measurement from the next pass on.  Tensors that OVERLAP a registered
                # one (one expert's slice of a stacked weight in the decode step) stay per-pass measurements: their packed pieces
                # would land on the registered tensor's, cut with another scale
                self._wkeys.append((p, key[2]))
                self._wdev = x.device
        return ptr_


def _drop_pending_on_failure(name):
    """A rejected entry point never wrote the maxima slots its producers were armed with (the C side disarms the sink itself,
    set_error): forget them, or a later GEMM keyed by the same (address, extent) would scale by a slot that still holds 0."""
    if _AMAX_REUSE is not None:
        _AMAX_REUSE.pending.clear()


_lib.FAILURE_HOOKS.append(_drop_pending_on_failure)

_AMAX_ATTN = os.environ.get("GAMER_AMAX_ATTN", "1") != "0"      # the attention kernels as producers (o, dv) - A/B switch


def _arm_sink(*outs):
    """outs: (tensor, (batch, stride, rows, cols, ld), accumulate) for the first / second output of the kernel launched next.
    With a maxima cache in effect and the split3 form selected, its slots are handed to that kernel (gamer_amax_sink)."""
    if _AMAX_REUSE is None or F32_MATMUL_TERMS != 3 or outs[0][0].dtype != torch.float32:
        return
    slots = [_AMAX_REUSE.preset(t, g, acc) for t, g, acc in outs]
    if slots[0] is None:
        return
    if len(slots) > 2:
        call("gamer_amax_sink3", slots[0], slots[1], slots[2])
    else:
        call("gamer_amax_sink", slots[0], slots[1] if len(slots) > 1 else None)


def scoped_amax(get_cache):
    """Decorator: `get_cache(*args)` (an amax_reuse or None) is the maxima cache in effect for the duration of the call."""
    import functools

    def deco(fn):
        @functools.wraps(fn)
        def wrapper(*args, **kwargs):
            cache = get_cache(*args)
            if cache is None:
                return fn(*args, **kwargs)
            with cache:
                return fn(*args, **kwargs)
        return wrapper
    return deco


def absmax_slot(x, batch, stride, rows, cols, ld, produced=False):
    """Device pointer of a word holding the bits of max |x| over `batch` matrices [rows, cols] (leading dimension ld).
    produced: x is about to be written by the kernel that gets the slot (it fills a zeroed word) - nothing is measured."""
    if _AMAX_REUSE is not None:
        if produced:
            _AMAX_REUSE.preset(x, (batch, stride, rows, cols, ld))
        return _AMAX_REUSE.slot(x, (batch, stride, rows, cols, ld))
    key = (x.device.index, stream_ptr())
    ring = _AMAX_RING.get(key)
    if ring is None:
        ring = _AMAX_RING[key] = [torch.zeros(_AMAX_SLOTS * AMAX_WORDS, dtype=torch.int32, device=x.device), 0]
    if ring[1] == _AMAX_SLOTS:
        ring[0].zero_()
        ring[1] = 0
    slot = ring[0].data_ptr() + 4 * AMAX_WORDS * ring[1]
    ring[1] += 1
    if not produced:
        call("gamer_absmax_f32", ptr(x), batch, stride, rows, cols, ld, slot, stream_ptr())
    return slot


def split3_planes(x, planes):
    """planes [3, n] bf16 <- the three exact bf16 pieces of x [n] fp32 (gamer_split3_planes)."""
    call("gamer_split3_planes", ptr(x), ptr(planes), x.numel(), planes.stride(0), stream_ptr())


# Ordered weight gradients (fp32 forms): the split-K chunks of gamer_gemm_f32 / _split store their partial tiles in a workspace
# and a second kernel adds them in chunk order (gamer_gemm_desc.wgrad_ws) instead of combining them with fp32 atomics, whose
# order varies from run to run.  ON by default since round 4: measured equal or faster than the atomics (247.4 vs 247.0 ms per
# step at per-GPU batch 1024, 33.10 vs 33.20 at 128 - 25 GB of float atomics per step become plain stores).
# GAMER_WGRAD_TWO_PASS=0 or `with ops.deterministic(False):` give the atomics form.
DETERMINISTIC_WGRAD = os.environ.get("GAMER_WGRAD_TWO_PASS", "1") != "0"
# The bf16 weight-gradient GEMM has the same ordered form (gamer_gemm_bf16_desc.wgrad_ws, same second pass).  There it measured
# 0.6 ms per step SLOWER than the atomics (104.2 against 103.6 ms at per-GPU batch 1024, equal at 128; the bf16 chunks are long and
# few, so there are few atomics to save), so it is opt-in: Engine(dtype="bf16", deterministic=True), GAMER_WGRAD_TWO_PASS_BF16=1.
DETERMINISTIC_WGRAD_BF16 = os.environ.get("GAMER_WGRAD_TWO_PASS_BF16", "0") == "1"
_WGRAD_WS = {}


class deterministic:
    """Scope: ordered (two-pass) weight gradients on / off for the fp32 forms; ``bf16`` (None = leave alone) likewise for the
    bf16 weight-gradient GEMM."""

    def __init__(self, on: bool = True, bf16=None):
        self.on, self.bf16 = bool(on), bf16

    def __enter__(self):
        global DETERMINISTIC_WGRAD, DETERMINISTIC_WGRAD_BF16
        self.prev, DETERMINISTIC_WGRAD = DETERMINISTIC_WGRAD, self.on
        self.prev16 = DETERMINISTIC_WGRAD_BF16
        if self.bf16 is not None:
            DETERMINISTIC_WGRAD_BF16 = bool(self.bf16)
        return self

    def __exit__(self, *exc):
        global DETERMINISTIC_WGRAD, DETERMINISTIC_WGRAD_BF16
        DETERMINISTIC_WGRAD, DETERMINISTIC_WGRAD_BF16 = self.prev, self.prev16
        return False


def _wgrad_workspace(device, floats: int) -> torch.Tensor:
    """grow-only scratch per device for the chunk partial tiles of the deterministic weight gradient"""
    t = _WGRAD_WS.get(device)
    if t is None or t.numel() < floats:
        _WGRAD_WS[device] = None
        t = _WGRAD_WS[device] = torch.empty(int(floats), dtype=torch.float32, device=device)
    return t


class split3_guard:
    """Context manager: the row-range guard of the split3 GEMMs on / off for the block (gamer_split3_guard in include/gamer_hip.h;
    on by default).  Tests turn it off to show what it guards against."""

    def __init__(self, on: bool):
        self.on = bool(on)

    def __enter__(self):
        self.prev = _lib.load().gamer_split3_guard(1 if self.on else 0)
        return self

    def __exit__(self, *exc):
        _lib.load().gamer_split3_guard(self.prev)
        return False


def set_f32_matmul(mode) -> int:
    """mode: "f32" | "split6" | "split9" (or 0 / 6 / 9); returns the previous setting."""
    global F32_MATMUL_TERMS
    prev = F32_MATMUL_TERMS
    terms = MATMUL_MODES[mode] if isinstance(mode, str) else int(mode)
    if terms not in (0, 3, 6, 9):
        raise ValueError(f"fp32 matmul mode {mode!r}: one of {sorted(MATMUL_MODES)}")
    F32_MATMUL_TERMS = terms
    return prev


def gemm(A, a_rs, a_ks, Bm, b_rs, b_ks, Cm, ldc, M, N, K, alpha=1.0, accumulate=False, groups=1, group_mode=0,
         group_offsets=None, strideB=0, strideC=0, kchunk=0, resid=None, row_map=None, p_drop=0.0, seed=0,
         rowdot=None, qknorm=None, c_amax=None, swiglu_bwd=None, group_div=0, sw_tbl=None, swiglu_fwd=None, norm=None, bias=None):
    """C[m][n] (=|+=) alpha * sum_k A(m,k) B(n,k); see gamer_gemm_desc in include/gamer_hip.h.  bf16 operands go to
    gamer_gemm_bf16 (k-contiguous x k-contiguous, or the token-major wgrad form; see gamer_gemm_bf16_desc).
    norm: dict(x, w, eps[, dst_rows, src_rows]) - A is first WRITTEN as the RMSNorm of x's rows (gamer_gemm_desc.norm_x);
    bias: dict(idx, q, k, v) - the row idx[m] of the tables q | k | v is added to C[m] (gamer_gemm_desc.bias_idx)."""
    if A.dtype == torch.bfloat16:
        if group_div > 1 or sw_tbl is not None or swiglu_fwd is not None or norm is not None or bias is not None:
            raise RuntimeError("group_div / sw_tbl / swiglu_fwd / norm / bias are options of the fp32 GEMM")
        return _gemm_bf16(A, a_rs, a_ks, Bm, b_rs, b_ks, Cm, ldc, M, N, K, alpha, accumulate, groups, group_mode,
                          group_offsets, strideB, strideC, kchunk, resid, row_map, p_drop, seed, rowdot, qknorm, swiglu_bwd)
    d = GemmDesc()
    d.A = ptr(A); d.a_rs = a_rs; d.a_ks = a_ks
    d.B = ptr(Bm); d.b_rs = b_rs; d.b_ks = b_ks
    d.C = ptr(Cm); d.ldc = ldc
    d.M = M; d.N = N; d.K = K
    d.alpha = alpha
    d.accumulate = 1 if accumulate else 0
    d.groups = groups
    d.group_mode = group_mode
    d.group_offsets = ptr(group_offsets)
    d.strideB = strideB; d.strideC = strideC
    d.kchunk = kchunk
    d.resid = ptr(resid)
    d.row_map = ptr(row_map)
    d.p_drop = p_drop
    d.seed = seed
    if rowdot is not None:                 # (other [M, ldc], out [M / S, N / 64, S], S): see gamer_gemm_desc
        d.rowdot_other, d.rowdot_out, d.rowdot_S = ptr(rowdot[0]), ptr(rowdot[1]), int(rowdot[2])
    if qknorm is not None:                 # the q|k|v epilogue: dict with the arguments of qknorm_rope_fwd
        q = qknorm
        d.qk_wq, d.qk_wk, d.qk_eps = ptr(q["wq"]), ptr(q["wk"]), float(q["eps"])
        d.qk_cos, d.qk_sin = ptr(q["cos"]), ptr(q["sin"])
        d.qk_bias_q, d.qk_bias_k, d.qk_bias_v = ptr(q.get("bias_q")), ptr(q.get("bias_k")), ptr(q.get("bias_v"))
        d.qk_act_idx, d.qk_pos_ids = ptr(q.get("act_idx")), ptr(q.get("pos_ids"))
        d.qk_q_rot, d.qk_k_rot = ptr(q["q_rot"]), ptr(q["k_rot"])
        d.qk_S, d.qk_nq, d.qk_nkv = int(q["S"]), int(q["nq"]), int(q["nkv"])
    if (c_amax is not None and _AMAX_REUSE is not None and F32_MATMUL_TERMS == 3 and group_mode == 0 and not accumulate
            and resid is None and qknorm is None and c_amax[1] % 64 == 0):
        # c_amax = (view of C from column col0 on, col0): the maximum of those columns comes out of this GEMM's epilogue into the
        # slot the next matrix product that reads the view (with this extent) will take - no gamer_absmax_f32 pass over it
        view, col0 = c_amax
        slot_c = _AMAX_REUSE.preset(view, (1, 0, M, N - col0, ldc))
        d.amax_c, d.amax_c_col0 = slot_c, int(col0)
    if swiglu_bwd is not None:
        # (gu, ld): C = d(hm) is consumed by the SwiGLU backward in the epilogue - gu <- d gate | d up - and never stored
        gu, ld_gu = swiglu_bwd
        d.sw_gu, d.sw_ld = ptr(gu), int(ld_gu)
        d.sw_tbl = ptr(sw_tbl)
        if _AMAX_REUSE is not None and F32_MATMUL_TERMS == 3 and ld_gu == 2 * N:
            d.amax_c, d.amax_c_col0 = _AMAX_REUSE.preset(gu, (1, 0, 1, M * ld_gu, M * ld_gu)), 0
    d.group_div = int(group_div)
    if norm is not None:
        nx = norm["x"]
        if group_mode != 0 or a_ks != 1 or b_ks != 1 or nx.dim() != 2 or nx.shape[0] < M or nx.shape[1] != K or not nx.is_contiguous():
            raise RuntimeError("gemm(norm=...): a Linear-forward GEMM whose rows are the RMSNorm of a dense [M, K] tensor")
        d.norm_x, d.norm_w, d.norm_eps = ptr(norm["x"]), ptr(norm["w"]), float(norm["eps"])
        d.norm_dst_rows, d.norm_src_rows = ptr(norm.get("dst_rows")), ptr(norm.get("src_rows"))
    if bias is not None:
        d.bias_idx, d.bias_q, d.bias_k, d.bias_v = ptr(bias["idx"]), ptr(bias["q"]), ptr(bias["k"]), ptr(bias["v"])
        d.bias_rows, d.bias_nq, d.bias_nkv = int(bias["q"].shape[0]), int(bias["q"].shape[1]), int(bias["k"].shape[1])
    if swiglu_fwd is not None:
        # (hm, tbl or None, row_group or None): C = gate | up AND hm = dropout(silu(gate + tg) * (up + tu)) from one call
        # (gamer_gemm_desc.sw_hm); the maximum of hm goes to the slot its consumer GEMM will take
        hm, tbl, row_group = swiglu_fwd
        d.sw_hm, d.sw_tbl, d.sw_row_group = ptr(hm), ptr(tbl), ptr(row_group)
        if _AMAX_REUSE is not None and F32_MATMUL_TERMS == 3:
            d.amax_c, d.amax_c_col0 = _AMAX_REUSE.preset(hm, (1, 0, 1, M * (N // 2), M * (N // 2))), 0
    if group_mode == 1 and DETERMINISTIC_WGRAD:
        n_chunks = (K + kchunk - 1) // kchunk + (groups if group_offsets is not None else 0)
        need = n_chunks * ((M + 127) // 128) * ((N + 127) // 128) * 16384
        ws = _wgrad_workspace(A.device, need)
        d.wgrad_ws, d.wgrad_ws_floats = ws.data_ptr(), ws.numel()
    if F32_MATMUL_TERMS == 3:
        # operand extents: A(m, k) at A + m a_rs + k a_ks, B(n, k) at B + n b_rs + k b_ks (one of each stride pair is 1)
        ga = (M, K, a_rs) if a_ks == 1 else (K, M, a_ks)
        gb = (N, K, b_rs) if b_ks == 1 else (K, N, b_ks)
        nb = (groups // max(1, int(group_div))) if (group_mode == 0 and groups > 1) else 1
        # (norm: A is produced by this call - its maximum too, into a fresh slot that the GEMMs reading A later take)
        d.amax_a = absmax_slot(A, 1, 0, *ga, produced=norm is not None)
        geom_b = (nb, strideB if nb > 1 else 0) + gb
        c = _AMAX_REUSE
        parent = c.plane_parent(Bm.data_ptr(), geom_b) if (c is not None and c.planes is not None and group_mode == 0) else None
        if parent is not None:
            # B is a VIEW (some columns of every row) of a parameter tensor with piece planes: the parent's maximum scales it (>= the
            # view's own; the planes were cut with it) and its pieces lie at the same offsets as the values
            d.amax_b = parent
            d.b_planes = c.planes.data_ptr() + (Bm.data_ptr() - c.stable_ranges[0][0])
            call("gamer_gemm_f32_split", C.byref(d), 3, stream_ptr())
            return
        d.amax_b = absmax_slot(Bm, *geom_b)
        if c is not None and c.planes is not None and group_mode == 0 and c._key(Bm.data_ptr(), geom_b) in c._plane_keys:
            # B is a parameter tensor whose fp16 piece planes were built at the start of this pass (same scale as amax_b gives)
            d.b_planes = c.planes.data_ptr() + (Bm.data_ptr() - c.stable_ranges[0][0])      # packed pieces at B's offsets
            if a_ks == 1 and b_ks == 1 and c._key(Bm.data_ptr(), geom_b) in c._tplane_keys:
                d.b_planes_t = c.planes_t.data_ptr() + (Bm.data_ptr() - c.stable_ranges[0][0])    # ... and of B^T
        call("gamer_gemm_f32_split", C.byref(d), 3, stream_ptr())
        return
    if F32_MATMUL_TERMS:
        if WEIGHT_PLANES is not None and group_mode == 0:
            base, nbytes, pl, stride = WEIGHT_PLANES
            off = Bm.data_ptr() - base
            if 0 <= off < nbytes:                       # B is a view of the engine's flat parameter buffer: hand over its planes
                d.b_planes, d.b_plane_stride = pl + off // 2, stride
        call("gamer_gemm_f32_split", C.byref(d), F32_MATMUL_TERMS, stream_ptr())
    else:
        call("gamer_gemm_f32", C.byref(d), stream_ptr())


def _gemm_bf16(A, a_rs, a_ks, Bm, b_rs, b_ks, Cm, ldc, M, N, K, alpha, accumulate, groups, group_mode, group_offsets,
               strideB, strideC, kchunk, resid, row_map, p_drop, seed, rowdot, qknorm=None, swiglu_bwd=None):
    if Bm.dtype != torch.bfloat16 or alpha != 1.0:
        raise RuntimeError("gamer_gemm_bf16 takes two bf16 operands and alpha = 1")
    d = GemmBf16Desc()
    if group_mode == 0:
        if a_ks != 1 or b_ks != 1:
            raise RuntimeError("bf16 GEMM: both operands must be k-contiguous (dgrad runs on the transposed weight copy)")
        d.lda, d.ldb = a_rs, b_rs
        want = torch.float32 if resid is not None else torch.bfloat16
    else:
        if a_rs != 1 or b_rs != 1:
            raise RuntimeError("bf16 wgrad: both operands must be token-major")
        d.lda, d.ldb = a_ks, b_ks
        want = torch.float32
    if Cm.dtype != want:
        raise RuntimeError(f"bf16 GEMM: C must be {want}, got {Cm.dtype}")
    d.A, d.B, d.C, d.ldc = ptr(A), ptr(Bm), ptr(Cm), ldc
    d.M, d.N, d.K = M, N, K
    d.accumulate = 1 if accumulate else 0
    d.groups, d.group_mode, d.group_offsets = groups, group_mode, ptr(group_offsets)
    d.strideB, d.strideC, d.kchunk = strideB, strideC, kchunk
    d.resid, d.row_map, d.p_drop, d.seed = ptr(resid), ptr(row_map), p_drop, seed
    if rowdot is not None:
        d.rowdot_other, d.rowdot_out, d.rowdot_S = ptr(rowdot[0]), ptr(rowdot[1]), int(rowdot[2])
    if qknorm is not None:                 # the q|k|v epilogue (AMP arithmetic of qknorm_rope_fwd on bf16 activations)
        q = qknorm
        d.qk_wq, d.qk_wk, d.qk_eps = ptr(q["wq"]), ptr(q["wk"]), float(q["eps"])
        d.qk_cos, d.qk_sin = ptr(q["cos"]), ptr(q["sin"])
        d.qk_bias_q, d.qk_bias_k, d.qk_bias_v = ptr(q.get("bias_q")), ptr(q.get("bias_k")), ptr(q.get("bias_v"))
        d.qk_act_idx, d.qk_pos_ids = ptr(q.get("act_idx")), ptr(q.get("pos_ids"))
        d.qk_q_rot, d.qk_k_rot = ptr(q["q_rot"]), ptr(q["k_rot"])
        d.qk_S, d.qk_nq, d.qk_nkv = int(q["S"]), int(q["nq"]), int(q["nkv"])
    if swiglu_bwd is not None:             # (gu, ld): see gamer_gemm_bf16_desc.sw_gu
        d.sw_gu, d.sw_ld = ptr(swiglu_bwd[0]), int(swiglu_bwd[1])
    if group_mode == 1 and DETERMINISTIC_WGRAD_BF16:
        n_chunks = (K + kchunk - 1) // kchunk + (groups if group_offsets is not None else 0)
        need = n_chunks * ((M + 127) // 128) * ((N + 127) // 128) * 16384
        ws = _wgrad_workspace(A.device, need)
        d.wgrad_ws, d.wgrad_ws_floats = ws.data_ptr(), ws.numel()
    call("gamer_gemm_bf16", C.byref(d), stream_ptr())


def linear_dgrad_t(dy, lddy, WT, ldwt, dx, lddx, M, K_out, N_in, accumulate=False, **grp):
    """dx[M,N_in] = dy[M,K_out] @ W[K_out,N_in] given WT = W^T [N_in, ldwt >= K_out] (k-contiguous on both sides: the
    form the bf16 path uses, against the transposed weight copy; K_out may include zero padding)."""
    gemm(dy, lddy, 1, WT, ldwt, 1, dx, lddx, M, N_in, K_out, accumulate=accumulate, **grp)


def qkv_fused_ok(x, M: int, N: int) -> bool:
    """The q|k|v GEMM can carry the per-head RMSNorm + RoPE epilogue: whole 128-row / 128-column tiles (fp32 or bf16)."""
    return x.dtype in (torch.float32, torch.bfloat16) and M % 128 == 0 and N % 128 == 0


def linear_fwd(x, ldx, W, ldw, y, ldy, M, N, K, accumulate=False, **grp):
    """y[M,N] = x[M,K] @ W[N,K]^T"""
    gemm(x, ldx, 1, W, ldw, 1, y, ldy, M, N, K, accumulate=accumulate, **grp)


def linear_dgrad(dy, lddy, W, ldw, dx, lddx, M, N_out, K_in, accumulate=False, **grp):
    """dx[M,K_in] = dy[M,N_out] @ W[N_out,K_in]"""
    gemm(dy, lddy, 1, W, 1, ldw, dx, lddx, M, K_in, N_out, accumulate=accumulate, **grp)


def pick_kchunk(rows: int, grouped: bool) -> int:
    """Token chunk per workgroup of the fp32 wgrad split.  Measured on MI355X at T = 517k (tools/wgrad_probe.py):
    1024 rows for the grouped (expert) form and 2048 for the plain one are within 3 % of the best for every
    shape on this path; 4k+ chunks lose 15-25 % to the tail (too few, too long workgroups)."""
    chunk = 1024 if grouped else 2048
    while chunk > 256 and rows < 64 * chunk:          # small problems: keep >= ~64 chunks
        chunk //= 2
    return chunk


# Token chunk of the split-K wgrad, measured once per (shape, dtype, matmul form) on first use: the best chunk depends on
# how tiles x chunks lands on the chip's 512 workgroup slots (tools/wgrad_probe.py: at 64,640 tokens the fixed rule loses
# 10-17 % on the o_proj, expert and head shapes; at 517k tokens 0-3 %).  GAMER_WGRAD_TUNE=0 keeps the fixed rules.
_WGRAD_TUNED = {}
_WGRAD_TUNE = os.environ.get("GAMER_WGRAD_TUNE", "1") != "0"


def _tune_allowed() -> bool:
    """On-line measurement only in single-process runs: under data parallelism every rank must pick the SAME chunk for
    a shape (the chunking is the fp32 summation partition of the weight gradient, and a sweep on one rank would skew
    step 0), so ranks use the shipped / file table (gamer_amd/wgrad_chunks.json, GAMER_WGRAD_TUNE_FILE) and the fixed
    rule - all deterministic functions of the shape."""
    if not _WGRAD_TUNE:
        return False
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            return False
    except Exception:                               # noqa: BLE001
        pass
    return int(os.environ.get("WORLD_SIZE", "1")) <= 1
# GAMER_WGRAD_TUNE_FILE=<json>: chunks measured by an earlier process are read from / added to this file (profiling runs:
# the sweep's launches would otherwise sit in the kernel statistics of the profiled step)
_WGRAD_TUNE_FILE = os.environ.get("GAMER_WGRAD_TUNE_FILE", "")


def _tune_key_str(key) -> str:
    return "|".join(str(k) for k in key)


_WGRAD_SHIPPED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wgrad_chunks.json")


def _load_tune_file():
    """Shipped table (chunks measured on MI355X for the bench shapes, tools/wgrad_table.py) overlaid by the user's file."""
    import json
    out = {}
    for path in (_WGRAD_SHIPPED, _WGRAD_TUNE_FILE):
        if path == _WGRAD_SHIPPED and os.environ.get("GAMER_WGRAD_IGNORE_SHIPPED", "0") not in ("", "0"):      # (tools/wgrad_table.py re-measures)
            continue
        if path and os.path.exists(path):
            try:
                with open(path) as f:
                    out.update({k: int(v) for k, v in json.load(f).items()})
            except (OSError, ValueError):
                pass
    return out


def _save_tune_file():
    """Atomic (temp file + rename): concurrent writers cannot leave a torn JSON behind."""
    import json
    import tempfile
    try:
        d = os.path.dirname(os.path.abspath(_WGRAD_TUNE_FILE))
        fd, tmp = tempfile.mkstemp(prefix=".wgrad_tune.", dir=d)
        with os.fdopen(fd, "w") as f:
            json.dump(_WGRAD_FILE_CACHE, f, indent=0)
        os.replace(tmp, _WGRAD_TUNE_FILE)
    except OSError:
        pass


_WGRAD_FILE_CACHE = _load_tune_file()


def _rule_kchunk(dy, rows, N_out, K_in, groups):
    if dy.dtype == torch.bfloat16:
        # bf16 tiles take 16x less matrix time than fp32 ones: chunks as long as possible (fewer fp32 atomics: every chunk
        # adds the whole 128 x 128 tile) while the grid still fills the chip's 512 workgroup slots once
        tiles = ((N_out + 127) // 128) * ((K_in + 127) // 128)
        per_group = max(1, rows // max(groups, 1))
        chunks = max(1, 512 // (tiles * max(groups, 1)))
        kchunk = min(16384, max(256, -(-per_group // chunks)))
        return (kchunk + 63) // 64 * 64
    return pick_kchunk(rows, groups > 1)


def _tune_kchunk(dy, lddy, x, ldx, dW, lddw, rows, N_out, K_in, groups, group_offsets, strideC):
    rule = _rule_kchunk(dy, rows, N_out, K_in, groups)
    if dy.dtype == torch.bfloat16:
        cands = {rule, 512, 1024, 2048, 4096, 8192, 16384, 1088, 2112, 3136, 4160, 6208}      # (multiples of 64; not only powers of two: see below)
    else:
        cands = {rule, 384, 512, 768, 1024, 1280, 1536, 2048, 3072, 4096}
        # ... and the chunks that make the grid a whole number of rounds of the chip's 512 workgroup slots (at per-GPU batch 128 a
        # power-of-two chunk leaves a quarter of the slots empty or starts a second, mostly empty round)
        tiles = ((N_out + 127) // 128) * ((K_in + 127) // 128)
        per_group = max(1, rows // max(groups, 1))
        for rounds in (1, 2, 3, 4):
            n_chunks = max(1, (512 * rounds) // (tiles * max(groups, 1)))
            c = (-(-per_group // n_chunks) + 31) // 32 * 32
            if 256 <= c <= 8192:
                cands.add(c)
        if F32_MATMUL_TERMS == 3 and N_out % 256 == 0 and K_in % 256 == 0:
            # the 256 x 256-tile kernel (csrc/gemm_wg.hip): one workgroup per CU, 256 slots; and chunks that are NOT a power of two -
            # with one, every workgroup's stream starts a multiple of 2 MB from the others' and they walk the memory channels in
            # step (measured: 2080 against 2048 tokens 5-15 % faster on the same shape, either kernel)
            tiles2 = (N_out // 256) * (K_in // 256)
            for rounds in (1, 2, 3, 4):
                n_chunks = max(1, (256 * rounds) // (tiles2 * max(groups, 1)))
                c = (-(-per_group // n_chunks) + 31) // 32 * 32
                if 256 <= c <= 8192:
                    cands.add(c)
            cands.update({1056, 2080, 3104, 4128})
    cands = sorted(c for c in cands if c <= max(256, rows))
    scratch = torch.zeros_like(dW)                 # the sweep must not touch the real gradient
    best, best_t = rule, float("inf")
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for c in cands:
        ts = []
        for it in range(4):
            s.record()
            gemm(dy, 1, lddy, x, 1, ldx, scratch, lddw, N_out, K_in, rows, groups=groups, group_mode=1,
                 group_offsets=group_offsets, strideC=strideC, kchunk=c)
            e.record()
            e.synchronize()
            if it:
                ts.append(s.elapsed_time(e))
        t = min(ts)
        if t < best_t * (0.98 if c != rule else 1.0):      # ties go to the smaller chunk / the rule
            best, best_t = c, t
    return best


def wgrad_rows_bucket(rows: int) -> int:
    """``tune_rows`` for callers whose row count changes from batch to batch (packed rows): rows rounded up to a step of about an
    eighth of their size, at least 4096, so that a handful of measured chunks serve every batch"""
    g = 1 << max(12, int(rows).bit_length() - 3)
    return -(-int(rows) // g) * g


def linear_wgrad(dy, lddy, x, ldx, dW, lddw, rows, N_out, K_in, groups=1, group_offsets=None, strideC=0, kchunk=None, tune_rows=None):
    """dW[N_out,K_in] += dy[rows,N_out]^T @ x[rows,K_in]   (dW must be initialised).  The token chunks of the split-K form are
    combined in chunk order through a workspace (two passes, the default in fp32; opt-in for bf16: ``deterministic``) or with fp32
    atomics (GAMER_WGRAD_TWO_PASS=0).  ``tune_rows``: the row count under which the measured chunk is kept (default: rows itself;
    a caller whose row count differs in every batch passes wgrad_rows_bucket(rows), or every step would measure again)."""
    if kchunk is None:
        key = (tune_rows or rows, N_out, K_in, groups, dy.dtype, F32_MATMUL_TERMS)
        kchunk = _WGRAD_TUNED.get(key)
        if kchunk is None and _tune_key_str(key) in _WGRAD_FILE_CACHE:
            kchunk = _WGRAD_TUNED[key] = _WGRAD_FILE_CACHE[_tune_key_str(key)]
        if kchunk is None:
            capturing = torch.cuda.is_current_stream_capturing()
            if rows >= 4096 and not capturing and _tune_allowed():
                kchunk = _tune_kchunk(dy, lddy, x, ldx, dW, lddw, rows, N_out, K_in, groups, group_offsets, strideC)
                if _WGRAD_TUNE_FILE:
                    _WGRAD_FILE_CACHE[_tune_key_str(key)] = int(kchunk)
                    _save_tune_file()
            else:
                kchunk = _rule_kchunk(dy, rows, N_out, K_in, groups)
            if not capturing:
                _WGRAD_TUNED[key] = kchunk
    gemm(dy, 1, lddy, x, 1, ldx, dW, lddw, N_out, K_in, rows, groups=groups, group_mode=1,
         group_offsets=group_offsets, strideC=strideC, kchunk=kchunk)


def qknorm_rope_fwd(qkv, S, nq, nkv, wq, wk, eps, cos_t, sin_t, q_rot, k_rot, bias_q=None, bias_k=None, bias_v=None,
                    act_idx=None, pos_ids=None):
    """pos_ids: int32 [T] RoPE table row per token (session model); None = position in the sequence."""
    T = qkv.shape[0]
    outs = [(q_rot, (1, 0, T, nq * 64, nq * 64), False), (k_rot, (1, 0, T, nkv * 64, nkv * 64), False)]
    if bias_v is not None:
        # the cross block: v + bias_v is written back into the v columns of q|k|v - their maximum is the attention's third operand
        outs.append((qkv[:, (nq + nkv) * 64:], (1, 0, T, nkv * 64, qkv.stride(0)), False))
    _arm_sink(*outs)
    call("gamer_qknorm_rope_fwd" + _sfx(qkv), ptr(qkv), T, S, nq, nkv, ptr(wq), ptr(wk), eps, ptr(cos_t), ptr(sin_t),
         ptr(bias_q), ptr(bias_k), ptr(bias_v), ptr(act_idx), ptr(q_rot), ptr(k_rot), ptr(pos_ids), stream_ptr())


def qknorm_partial_numel(nb1: int = 0) -> int:
    """fp32 scratch of qknorm_rope_bwd that never limits its wave count (see gamer_hip.h)."""
    return 8192 * (1 + nb1) * 64


def qknorm_rope_bwd(qkv, dq_rot, dk_rot, S, nq, nkv, wq, wk, eps, cos_t, sin_t, dqkv, dwq, dwk, bias_q=None,
                    bias_k=None, act_idx=None, nb1=0, dbias_q=None, dbias_k=None, dbias_v=None, pos_ids=None,
                    partial=None):
    """partial: fp32 scratch for the per-wave sums of the weight / bias gradients (allocated here when None).
    dwq, dwk and dbias_q / _k / _v are ADDED to (`+=`, in a fixed order: the same bits on every call) - zero them for a plain
    gradient; dqkv[:, :q|k] is overwritten; dqkv[:, v] must hold dV (the cross call sums it into dbias_v) and is left as it is."""
    T = qkv.shape[0]
    if partial is None:
        partial = torch.empty(qknorm_partial_numel(nb1), dtype=torch.float32, device=qkv.device)
    # the q and k columns of d(q|k|v) are written here, the v columns by the attention backward before: its slot, if it opened one
    _arm_sink((dqkv, (1, 0, T, dqkv.shape[1], dqkv.stride(0)), "only"))
    call("gamer_qknorm_rope_bwd" + _sfx(qkv), ptr(qkv), ptr(dq_rot), ptr(dk_rot), T, S, nq, nkv, ptr(wq), ptr(wk), eps,
         ptr(cos_t), ptr(sin_t), ptr(bias_q), ptr(bias_k), ptr(act_idx), nb1, ptr(dqkv), ptr(dwq), ptr(dwk),
         ptr(dbias_q), ptr(dbias_k), ptr(dbias_v), ptr(pos_ids), ptr(partial), partial.numel(), stream_ptr())


def attn_row_order(row_empty, perm, tile_kind, tile_maxpos):
    B, S = row_empty.shape
    call("gamer_attn_row_order", ptr(row_empty), B, S, ptr(perm), ptr(tile_kind), ptr(tile_maxpos), stream_ptr())


def attn_fwd(q, ldq, k, ldk, v, ldv, kl, ql, row_empty, tile_empty, B, S, nq, nkv, scale, p_drop, seed, o, lse,
             order=None, uniform_len=0, q_span=None):
    """order = (perm, tile_kind, tile_maxpos) from attn_row_order, or None for the natural row order.
    uniform_len: see include/gamer_hip.h (0 = training semantics).
    q_span: int32 [B,S,4] per-query key spans from session_spans (session model), None = plain causal."""
    pm, tk, tm = order if order is not None else (None, None, None)
    call("gamer_attn_fwd", ptr(q), ldq, ptr(k), ldk, ptr(v), ldv, ptr(kl), ptr(ql), ptr(row_empty), ptr(tile_empty),
         B, S, nq, nkv, scale, p_drop, seed, ptr(o), ptr(lse), ptr(pm), ptr(tk), ptr(tm), uniform_len, ptr(q_span),
         stream_ptr())


def attn_bwd(q, ldq, k, ldk, v, ldv, o, d_o, lse, kl, ql, row_empty, tile_empty, B, S, nq, nkv, scale, p_drop, seed,
             delta, dq, lddq, dk, lddk, dv, lddv, order=None, ds_work=None, q_span=None, delta_ready=False):
    """ds_work: optional fp32 scratch of attn_ds_work_numel(B, S, nq) elements (dS spill, see gamer_hip.h)."""
    pm, tk, tm = order if order is not None else (None, None, None)
    call("gamer_attn_bwd", ptr(q), ldq, ptr(k), ldk, ptr(v), ldv, ptr(o), ptr(d_o), ptr(lse), ptr(kl), ptr(ql),
         ptr(row_empty), ptr(tile_empty), B, S, nq, nkv, scale, p_drop, seed, ptr(delta), ptr(dq), lddq, ptr(dk),
         lddk, ptr(dv), lddv, ptr(pm), ptr(tk), ptr(tm), ptr(ds_work), ptr(q_span),
         1 if (delta_ready and ds_work is not None) else 0, stream_ptr())


def attn_operand_maxima(q, ldq, k, ldk, v, ldv, T, nq, nkv, d_o=None):
    """Slots with the maxima of the attention operands (the three-product fp16 form): measured here unless their producers
    left them in the cache in effect (ops.amax_reuse)."""
    sl = [absmax_slot(q, 1, 0, T, nq * 64, ldq), absmax_slot(k, 1, 0, T, nkv * 64, ldk), absmax_slot(v, 1, 0, T, nkv * 64, ldv)]
    sl.append(absmax_slot(d_o, 1, 0, T, nq * 64, nq * 64) if d_o is not None else None)
    return sl


def attn_fwd_split(q, ldq, k, ldk, v, ldv, kl, ql, row_empty, B, S, nq, nkv, scale, p_drop, seed, o, lse, order=None,
                   h2=False, uniform_len=0, q_span=None):
    """gamer_attn_fwd with its products on the 16-bit matrix pipe; training semantics.  h2 = False: exact three-way bf16
    cuts, six piece products; h2 = True: two-way fp16 cuts scaled per tensor, three piece products (gamer_attn_split_amax)."""
    pm, tk, tm = order if order is not None else (None, None, None)
    if h2:
        call("gamer_attn_split_amax", *attn_operand_maxima(q, ldq, k, ldk, v, ldv, B * S, nq, nkv))
    if _AMAX_ATTN:
        _arm_sink((o, (1, 0, 1, B * S * nq * 64, B * S * nq * 64), False))
    call("gamer_attn_fwd_split", ptr(q), ldq, ptr(k), ldk, ptr(v), ldv, ptr(kl), ptr(ql), ptr(row_empty), B, S, nq, nkv,
         scale, p_drop, seed, ptr(o), ptr(lse), ptr(pm), ptr(tk), ptr(tm), int(uniform_len), ptr(q_span), stream_ptr())


def attn_bwd_split(q, ldq, k, ldk, v, ldv, o, d_o, lse, kl, ql, row_empty, tile_empty, B, S, nq, nkv, scale, p_drop, seed,
                   delta, dq, lddq, dk, lddk, dv, lddv, order=None, delta_ready=False, ds_work=None, dv_of=None, h2=False,
                   q_span=None):
    """gamer_attn_bwd with its products on the bf16 pipe; delta_ready: `delta` already holds dO.O; ds_work: the dS spill
    scratch of attn_bwd (None = recompute form); dv_of: the d(q|k|v) tensor whose v columns `dv` is (its maximum is then
    collected by the kernels that write it: this one and qknorm_rope_bwd)."""
    pm, tk, tm = order if order is not None else (None, None, None)
    if h2:           # the three-product fp16 form (see attn_fwd_split)
        call("gamer_attn_split_amax", *attn_operand_maxima(q, ldq, k, ldk, v, ldv, B * S, nq, nkv, d_o=d_o))
    if dv_of is not None and _AMAX_ATTN:
        _arm_sink((dv_of, (1, 0, dv_of.shape[0], dv_of.shape[1], dv_of.stride(0)), False))
    call("gamer_attn_bwd_split", ptr(q), ldq, ptr(k), ldk, ptr(v), ldv, ptr(o), ptr(d_o), ptr(lse), ptr(kl), ptr(ql),
         ptr(row_empty), ptr(tile_empty), B, S, nq, nkv, scale, p_drop, seed, ptr(delta), ptr(dq), lddq, ptr(dk), lddk, ptr(dv),
         lddv, ptr(pm), ptr(tk), ptr(tm), 1 if delta_ready else 0, ptr(ds_work), ptr(q_span), stream_ptr())


def attn_fwd_bf16(q, ldq, k, ldk, v, ldv, kl, ql, B, S, nq, nkv, scale, p_drop, seed, o, lse, q_span=None, order=None):
    """bf16 attention (empty rows -> 0, see gamer_attn_fwd_bf16 in include/gamer_hip.h).
    order = (perm, tile_maxpos, row_empty): visit the query rows through the row order of attn_row_order."""
    perm, tmax, rempty = order if order is not None else (None, None, None)
    call("gamer_attn_fwd_bf16", ptr(q), ldq, ptr(k), ldk, ptr(v), ldv, ptr(kl), ptr(ql), B, S, nq, nkv, scale, p_drop,
         seed, ptr(o), ptr(lse), ptr(q_span), ptr(perm), ptr(tmax), ptr(rempty), stream_ptr())


def attn_bwd_bf16(q, ldq, k, ldk, v, ldv, o, d_o, lse, kl, ql, B, S, nq, nkv, scale, p_drop, seed, delta, dq, lddq, dk,
                  lddk, dv, lddv, q_span=None, delta_ready=False, order=None):
    perm, tmax, rempty = order if order is not None else (None, None, None)
    call("gamer_attn_bwd_bf16", ptr(q), ldq, ptr(k), ldk, ptr(v), ldv, ptr(o), ptr(d_o), ptr(lse), ptr(kl), ptr(ql),
         B, S, nq, nkv, scale, p_drop, seed, ptr(delta), ptr(dq), lddq, ptr(dk), lddk, ptr(dv), lddv, ptr(q_span),
         1 if delta_ready else 0, ptr(perm), ptr(tmax), ptr(rempty), stream_ptr())


def cast_params_bf16(flat, out, out_t, table, n_entries, n_tiles):
    """bf16 (and transposed bf16) operand copies of the fp32 master parameters; table from engine.Bf16Shadow."""
    call("gamer_cast_params_bf16", ptr(flat), ptr(out), ptr(out_t), ptr(table), n_entries, n_tiles, stream_ptr())


def attn_ds_work_numel(B, S, nq):
    n = (S + 31) // 32
    return B * nq * n * n * 1024


def residual_dropout_fwd(x, delta, p, seed, src_rows=None, out=None):
    """out = x + drop(delta[src]); out defaults to x (in place)."""
    T, H = x.shape
    call("gamer_residual_dropout_fwd", ptr(x), ptr(delta), ptr(src_rows), T, H, p, seed,
         ptr(out if out is not None else x), stream_ptr())


def residual_dropout_bwd(dx, p, seed, ddelta, src_rows=None):
    T, H = dx.shape
    call("gamer_residual_dropout_bwd", ptr(dx), ptr(src_rows), T, H, p, seed, ptr(ddelta), stream_ptr())


def swiglu_fwd(g, u, n, p, seed, hm):
    _arm_sink((hm, (1, 0, 1, n, n), False))
    call("gamer_swiglu_fwd" + _sfx(g), ptr(g), ptr(u), n, p, seed, ptr(hm), stream_ptr())


def swiglu_bwd(g, u, dhm, n, p, seed):
    _arm_sink((g, (1, 0, 1, n, n), False), (u, (1, 0, 1, n, n), False))
    call("gamer_swiglu_bwd" + _sfx(g), ptr(g), ptr(u), ptr(dhm), n, p, seed, stream_ptr())


def swiglu_fwd_ld(gu, ld, T, I, p, seed, hm):
    """hm[T, I] = drop(silu(gu[:, :I]) * gu[:, I:2I]) on the output of the fused gate|up projection (row stride ld)."""
    _arm_sink((hm, (1, 0, 1, T * I, T * I), False))
    call("gamer_swiglu_fwd_ld" + _sfx(gu), ptr(gu), ld, T, I, p, seed, ptr(hm), stream_ptr())


def swiglu_bwd_ld(gu, ld, T, I, dhm, p, seed):
    """In place: gu[:, :I] <- d gate, gu[:, I:2I] <- d up.  The maximum of the whole [T, 2I] gradient goes to ONE slot (it is
    one GEMM operand from here on) when the buffer is contiguous (ld == 2 I)."""
    if ld == 2 * I:
        geom = (1, 0, 1, T * ld, T * ld)
        _arm_sink((gu, geom, False), (gu, geom, True))
    call("gamer_swiglu_bwd_ld" + _sfx(gu), ptr(gu), ld, T, I, ptr(dhm), p, seed, stream_ptr())


def silu_fwd_ld(h, ld, T, I, p, seed, hm):
    """hm[T, I] = drop(silu(h[:, :I])) on the output of a non-gated FFN's wi projection (row stride ld; mlp_type "PBATransformer")."""
    _arm_sink((hm, (1, 0, 1, T * I, T * I), False))
    call("gamer_silu_fwd_ld" + _sfx(h), ptr(h), ld, T, I, p, seed, ptr(hm), stream_ptr())


def silu_bwd_ld(h, ld, T, I, dhm, p, seed):
    """In place: h[:, :I] <- drop_mask * dhm * silu'(h)."""
    if ld == I:
        _arm_sink((h, (1, 0, 1, T * I, T * I), False))
    call("gamer_silu_bwd_ld" + _sfx(h), ptr(h), ld, T, I, ptr(dhm), p, seed, stream_ptr())


def swiglu_fwd_ld_tbl(gu, ld, T, I, p, seed, hm, tbl, row_group):
    """hm = drop(silu(g) * u) with g | u = gu[t] + tbl[row_group[t]] (fp32; see gamer_inject_table_fwd)."""
    _arm_sink((hm, (1, 0, 1, T * I, T * I), False))
    call("gamer_swiglu_fwd_ld_tbl", ptr(gu), ld, T, I, p, seed, ptr(hm), ptr(tbl), ptr(row_group), stream_ptr())


def swiglu_bwd_ld_tbl(gu, ld, T, I, dhm, p, seed, tbl, row_group):
    if ld == 2 * I:
        _arm_sink((gu, (1, 0, 1, T * ld, T * ld), False), (gu, (1, 0, 1, T * ld, T * ld), True))
    call("gamer_swiglu_bwd_ld_tbl", ptr(gu), ld, T, I, ptr(dhm), p, seed, ptr(tbl), ptr(row_group), stream_ptr())


def pba_router(ids, decoder, num_positions, n_items, moe_behavior_only, use_behavior_token, behavior_lut, nb1, num_experts, pad_id,
               eos_id, expert, beh_idx, key, bad_token):
    """PBATransformer's encoder (``decoder=False``) or decoder router in one launch (gamer_pba_router): ids int64 [B, S] -> expert,
    beh_idx and (or None) key = expert * nb1 + beh_idx, int32 [B, S]; ``bad_token`` int32 [1] is added to, never cleared.
    ``behavior_lut``: int32 [vocab] on the device (-1: no behaviour token), None without behaviour tokens."""
    B, S = ids.shape
    _chk(ids, torch.int64, "input_ids")
    for name, t in (("expert", expert), ("beh_idx", beh_idx), ("key", key), ("bad_token", bad_token), ("behavior_lut", behavior_lut)):
        if t is not None:
            _chk(t, torch.int32, name)
    if expert.numel() != B * S or beh_idx.numel() != B * S or (key is not None and key.numel() != B * S):
        raise ValueError(f"pba_router: outputs of {B * S} entries")
    call("gamer_pba_router", ptr(ids), B, S, 1 if decoder else 0, num_positions, n_items, 1 if moe_behavior_only else 0,
         1 if use_behavior_token else 0, ptr(behavior_lut), behavior_lut.numel() if behavior_lut is not None else 0, nb1, num_experts,
         pad_id, eos_id, ptr(expert), ptr(beh_idx), ptr(key), ptr(bad_token), stream_ptr())


def _relu_tbl_args(name, pre, ld, T, I, other, tbl, row_group, n_groups):
    _chk(pre, torch.float32, "pre"), _chk(other, torch.float32, name)
    if pre.numel() < (T - 1) * ld + I or other.numel() < T * I:
        raise ValueError(f"relu_tbl: pre holds {pre.numel()} and {name} {other.numel()} values (T={T}, I={I}, ld={ld})")
    if (tbl is None) != (row_group is None):
        raise ValueError("relu_tbl: tbl and row_group come together")
    if tbl is not None:
        _chk(tbl, torch.float32, "tbl"), _chk(row_group, torch.int32, "row_group")
        if tbl.numel() < n_groups * I or row_group.numel() < T:
            raise ValueError(f"relu_tbl: tbl [{n_groups}, {I}] and row_group [{T}] (got {tbl.numel()} and {row_group.numel()} entries)")


def relu_tbl_fwd(pre, ld, T, I, p, seed, act, tbl=None, row_group=None, n_groups=0):
    """act [T, I] = drop(relu(pre[:, :I] + tbl[row_group])) (gamer_relu_tbl_fwd; pre has row stride ld; tbl None: no table)."""
    _relu_tbl_args("act", pre, ld, T, I, act, tbl, row_group, n_groups)
    call("gamer_relu_tbl_fwd", ptr(pre), ld, T, I, p, seed, ptr(act), ptr(tbl), ptr(row_group), n_groups, stream_ptr())


def relu_tbl_bwd(pre, ld, T, I, dact, p, seed, tbl=None, row_group=None, n_groups=0):
    """In place: pre[:, :I] <- drop_mask * dact * (pre + tbl[row_group] > 0) (gamer_relu_tbl_bwd)."""
    _relu_tbl_args("dact", pre, ld, T, I, dact, tbl, row_group, n_groups)
    call("gamer_relu_tbl_bwd", ptr(pre), ld, T, I, ptr(dact), p, seed, ptr(tbl), ptr(row_group), n_groups, stream_ptr())


def inject_table_fwd(Eb, W, ldw, col0, E, twoI, tbl):
    """tbl [E * NB1, 2I] <- the behaviour-embedding share of the gate|up projection per (expert, behaviour) (gamer_inject_table_fwd)."""
    NB1, EB = Eb.shape
    call("gamer_inject_table_fwd", ptr(Eb), ptr(W), ldw, col0, E, twoI, NB1, EB, ptr(tbl), stream_ptr())


def segment_colsum_ws_floats(rows, cols, nseg) -> int:
    return int(_lib.load().gamer_segment_colsum_ws_floats(rows, cols, nseg))


def segment_colsum(x, ld, rows, cols, offsets, nseg, ws, out):
    call("gamer_segment_colsum", ptr(x), ld, rows, cols, ptr(offsets), nseg, ptr(ws), ws.numel(), ptr(out), stream_ptr())


def inject_table_bwd(seg, Eb, W, ldw, col0, E, twoI, dW, dEb, scratch):
    NB1, EB = Eb.shape
    call("gamer_inject_table_bwd", ptr(seg), ptr(Eb), ptr(W), ldw, col0, E, twoI, NB1, EB, ptr(dW), ptr(dEb), ptr(scratch), stream_ptr())


def silu_gate_fwd(a, gate, out, resid=None, p=0.0, seed=0):
    """out = a * silu(gate), or resid + dropout(a * silu(gate)) when resid is given (fused residual add)."""
    call("gamer_silu_gate_fwd" + _sfx(a), ptr(a), ptr(gate), a.numel(), ptr(out), ptr(resid), p, seed, stream_ptr())


def silu_gate_bwd(a, gate, dout, da, dgate, p=0.0, seed=0):
    """p > 0: dout is the residual-stream gradient and the forward's dropout mask (seed) is applied to it first."""
    _arm_sink((da, (1, 0, 1, a.numel(), a.numel()), False), (dgate, (1, 0, 1, a.numel(), a.numel()), False))
    call("gamer_silu_gate_bwd" + _sfx(a), ptr(a), ptr(gate), ptr(dout), a.numel(), ptr(da), ptr(dgate), p, seed, stream_ptr())


def check_labels(labels, V, ignore_index, bad_label):
    call("gamer_check_labels", ptr(labels), labels.numel(), V, ignore_index, ptr(bad_label), stream_ptr())


def ce_fwd(logits, ldl, labels, V, temperature, ignore_index, lse, row_loss, loss_sum, count):
    B, S = labels.shape
    call("gamer_ce_fwd" + _sfx(logits), ptr(logits), ldl, ptr(labels), B, S, V, temperature, ignore_index, ptr(lse), ptr(row_loss),
         ptr(loss_sum), ptr(count), stream_ptr())


def ce_bwd(logits, ldl, labels, V, temperature, ignore_index, lse, count_dev, denom_host, dloss, dloss_dev=None):
    """dloss_dev: optional fp32 device scalar multiplied into dloss (autograd's incoming gradient, no host read)."""
    B, S = labels.shape
    _arm_sink((logits, (1, 0, B * S, V, ldl), False))
    call("gamer_ce_bwd" + _sfx(logits), ptr(logits), ldl, ptr(labels), B, S, V, temperature, ignore_index, ptr(lse), ptr(count_dev),
         float(denom_host), float(dloss), ptr(dloss_dev), stream_ptr())


def sumsq(g, partial):
    call("gamer_sumsq", ptr(g), g.numel(), ptr(partial), partial.numel(), stream_ptr())


def adamw(p, g, m, v, n_decay, lr, beta1, beta2, eps, weight_decay, step, max_norm, grad_scale, partial, norm_out):
    call("gamer_adamw", ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), n_decay, lr, beta1, beta2, eps, weight_decay,
         step, max_norm, grad_scale, ptr(partial), partial.numel(), ptr(norm_out), stream_ptr())


def fill(t, value):
    call("gamer_fill_f32", ptr(t), t.numel(), float(value), stream_ptr())


# ---- evaluation path: trie-constrained beam-search scoring ---------------------------------------
def trie_logprobs(logits2d, row_index, beam_score, node, child_start, child_tok, V, scores):
    """scores[n] = log_softmax(logits2d[row_index[n], :V]) + beam_score[n] on the child tokens of trie node[n],
    -inf elsewhere."""
    N = row_index.numel()
    call("gamer_trie_logprobs", ptr(logits2d), logits2d.stride(0), ptr(row_index), ptr(beam_score), ptr(node),
         ptr(child_start), ptr(child_tok), N, V, ptr(scores), stream_ptr())


def trie_advance(node, token, child_start, child_tok, child_node, out):
    call("gamer_trie_advance", ptr(node), ptr(token), ptr(child_start), ptr(child_tok), ptr(child_node),
         node.numel(), ptr(out), stream_ptr())


def kv_append(k, v, kg, vg, g):
    """kg / vg [N, tmax, C] <- k [N, C], v [N, C] (row-strided views) at generated position g."""
    N, tmax, C = kg.shape
    call("gamer_kv_append", ptr(k), k.stride(0), ptr(v), v.stride(0), ptr(kg), ptr(vg), kg.stride(1), tmax, g, N, C, stream_ptr())


def attn_decode(q, kp, vp, key_ok, kg, vg, t, gen_ok, uniform, B, nb, L0, nq, nkv, scale, o, amax=None):
    """One new token per beam against the prompt cache (per sample) + generated cache (per beam).
    amax = (slot of max |kp|, slot of max |vp|): the three-piece fp16 form (gamer_attn_decode_split)."""
    tmax = kg.shape[1]
    if amax is not None:
        n = o.numel()
        _arm_sink((o, (1, 0, 1, n, n), False))
        call("gamer_attn_decode_split", ptr(q), q.stride(0), ptr(kp), kp.stride(0), ptr(vp), vp.stride(0), ptr(key_ok), ptr(kg),
             ptr(vg), kg.stride(1), tmax, t, 1 if gen_ok else 0, ptr(uniform), B, nb, L0, nq, nkv, scale, ptr(o), amax[0], amax[1],
             stream_ptr())
        return
    call("gamer_attn_decode", ptr(q), q.stride(0), ptr(kp), kp.stride(0), ptr(vp), vp.stride(0), ptr(key_ok), ptr(kg),
         ptr(vg), kg.stride(1), tmax, t, 1 if gen_ok else 0, ptr(uniform), B, nb, L0, nq, nkv, scale, ptr(o),
         stream_ptr())


def attn_candidates(q, kp, vp, key_ok, kg, vg, t, gen_ok, uniform, B, nb, L0, nq, nkv, scale, o):
    """attn_decode for any number ``nb`` of rows per sample (gamer_attn_candidates: the waves of a workgroup share the staged
    prompt tiles; fp32 MFMA in every fp32 matmul form): the step attention of ``decode.score_items``."""
    for name, x in (("q", q), ("kp", kp), ("vp", vp), ("kg", kg), ("vg", vg), ("o", o)):
        _chk(x, torch.float32, name)
    _chk(key_ok, torch.int32, "key_ok")
    call("gamer_attn_candidates", ptr(q), q.stride(0), ptr(kp), kp.stride(0), ptr(vp), vp.stride(0), ptr(key_ok), ptr(kg),
         ptr(vg), kg.stride(1), kg.shape[1], t, 1 if gen_ok else 0, ptr(uniform), B, nb, L0, nq, nkv, scale, ptr(o),
         stream_ptr())


def token_logprob(logits2d, row_index, token, V, out, accumulate=False):
    """out[n] (+)= log_softmax(logits2d[row_index[n], :V])[token[n]] (row_index None: row n), gamer_token_logprob."""
    _chk(token, torch.int64, "token")
    call("gamer_token_logprob", ptr(logits2d), logits2d.stride(0), ptr(row_index), ptr(token), token.numel(), V,
         1 if accumulate else 0, ptr(out), stream_ptr())


def kv_append_bf16(k, v, kg, vg, g):
    """kv_append on bf16 rows (the bf16 engine's generated self cache)."""
    for name, x in (("k", k), ("v", v), ("kg", kg), ("vg", vg)):
        _chk(x, torch.bfloat16, name)
    N, tmax, C = kg.shape
    call("gamer_kv_append_bf16", ptr(k), k.stride(0), ptr(v), v.stride(0), ptr(kg), ptr(vg), kg.stride(1), tmax, g, N, C, stream_ptr())


def attn_decode_bf16(q, kp, vp, key_ok, kg, vg, t, gen_ok, B, nb, L0, nq, nkv, scale, o):
    """attn_decode on a bf16 cache with the bf16 attention's semantics (gamer_attn_decode_bf16): a row with no allowed key gives
    zeros - no ``uniform`` -, and with ``gen_ok`` False (a cross block) kg / vg are not read.  q [N, >= nq*64] and o [N, nq*64] bf16."""
    for name, x in (("q", q), ("kp", kp), ("vp", vp), ("kg", kg), ("vg", vg), ("o", o)):
        _chk(x, torch.bfloat16, name)
    _chk(key_ok, torch.int32, "key_ok")
    call("gamer_attn_decode_bf16", ptr(q), q.stride(0), ptr(kp), kp.stride(0), ptr(vp), vp.stride(0), ptr(key_ok), ptr(kg), ptr(vg),
         kg.stride(1), kg.shape[1], t, 1 if gen_ok else 0, B, nb, L0, nq, nkv, scale, ptr(o), stream_ptr())


# ---- post-LN encoder of the discriminative baselines (SeqRec/modules/layers/transformer.py) --------------------
ACTIVATIONS ={"none": 0, "relu": 1, "gelu": 2, "swish": 3, "tanh": 4, "sigmoid": 5, "elu": 6}


def bias_act_fwd(x, bias, act: int, y=None):
    """x[T,N] <- x + bias in place; y = act(x + bias) when given."""
    T, N = x.shape
    call("gamer_bias_act_fwd", ptr(x), ptr(bias), T, N, act, ptr(y), stream_ptr())


def bias_act_bwd(pre, dy, act: int, dx, db_partial):
    T, N = dy.shape
    call("gamer_bias_act_bwd", ptr(pre), ptr(dy), T, N, act, ptr(dx), ptr(db_partial), db_partial.shape[0], stream_ptr())


def layernorm_fwd(x, res, w, b, eps, v_out, y, mean, rstd):
    T, H = x.shape
    call("gamer_layernorm_fwd", ptr(x), ptr(res), ptr(w), ptr(b), T, H, eps, ptr(v_out), ptr(y), ptr(mean), ptr(rstd),
         stream_ptr())


def layernorm_bwd(v, w, mean, rstd, dy, dx, dw_partial, db_partial):
    T, H = v.shape
    call("gamer_layernorm_bwd", ptr(v), ptr(w), ptr(mean), ptr(rstd), ptr(dy), T, H, ptr(dx), ptr(dw_partial),
         ptr(db_partial), dw_partial.shape[0], stream_ptr())


def _mask_strides(mask, B, H, S):
    """element strides of an additive mask broadcastable to [B,H,S,S] (size-1 dims get stride 0)"""
    if mask is None:
        return None, None
    if mask.dim() != 4 or mask.dtype != torch.float32:
        raise RuntimeError("attention mask must be a 4-d float32 tensor broadcastable to [B, heads, S, S]")
    want = (B, H, S, S)
    st = []
    for d in range(4):
        if mask.shape[d] == want[d] and mask.shape[d] != 1:
            st.append(mask.stride(d))
        elif mask.shape[d] == 1:
            st.append(0)
        else:
            raise RuntimeError(f"attention mask shape {tuple(mask.shape)} does not broadcast to {want}")
    return mask, (C.c_int64 * 4)(*st)


def attn_dense_fwd(q, k, v, mask, B, S, H, dh, scale, p_drop, seed, o, lse):
    m, st = _mask_strides(mask, B, H, S)
    call("gamer_attn_dense_fwd", ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v), v.stride(0), ptr(m), st, B, S, H, dh,
         scale, p_drop, seed, ptr(o), o.stride(0), ptr(lse), stream_ptr())


def attn_dense_bwd(q, k, v, mask, B, S, H, dh, scale, p_drop, seed, o, d_o, lse, dq, dk, dv):
    m, st = _mask_strides(mask, B, H, S)
    call("gamer_attn_dense_bwd", ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v), v.stride(0), ptr(m), st, B, S, H, dh,
         scale, p_drop, seed, ptr(o), ptr(d_o), o.stride(0), ptr(lse), ptr(dq), dq.stride(0), ptr(dk), dk.stride(0),
         ptr(dv), dv.stride(0), stream_ptr())


# ---- catalogue-wide head of the discriminative baselines (csrc/catalog.hip) --------------------------------------------------
_CAT_WS = {}


def _ws(key, device, nbytes):
    """a cached uint8 device workspace of at least nbytes (one per (key, device))"""
    ws = _CAT_WS.get((key, device))
    if ws is None or ws.numel() < nbytes:
        _CAT_WS[(key, device)] = None
        ws = _CAT_WS[(key, device)] = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)
    return ws


def _dense(t, dtype, name):
    """a contiguous device tensor of dtype (the kernels read flat rows)"""
    _chk(t, dtype, name)
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
    return t


def _rows(h, row_idx):
    """(row-strided 2-d view of h, index pointer, idx64, R)"""
    _chk(h, torch.float32, "h")
    h2 = h.reshape(-1, h.shape[-1])
    if h2.stride(1) != 1:
        raise RuntimeError("catalogue head: h rows must be contiguous")
    if row_idx is None:
        return h2, None, 0, h2.shape[0]
    if row_idx.dtype not in (torch.int32, torch.int64) or not row_idx.is_contiguous():
        raise RuntimeError("catalogue head: row_idx must be a contiguous int32 / int64 tensor")
    return h2, row_idx, 1 if row_idx.dtype == torch.int64 else 0, row_idx.numel()


def _head(E, biased, bias, V):
    """(V, H, the bias argument of the entry point): the head scores the first V rows of E, all of them by default (BERT4Rec's
    table ends with the <MASK> row); only the _bias entry points take a bias"""
    V = E.shape[0] if V is None else int(V)
    if not 0 < V <= E.shape[0]:
        raise RuntimeError(f"catalogue head: V = {V} outside (0, {E.shape[0]}]")
    if bias is not None and _dense(bias, torch.float32, "bias").numel() < V:
        raise RuntimeError(f"catalogue head: bias must hold V = {V} values")
    return V, E.shape[1], ((ptr(bias),) if biased else ())


def _catalog_ce_fwd(biased, h, row_idx, E, bias, target, lse, loss, bad, V):
    name = "catalog_ce_bias_fwd" if biased else "catalog_ce_fwd"
    h2, idx, idx64, R = _rows(h, row_idx)
    _dense(E, torch.float32, "E"), _dense(target, torch.int64, "target"), _dense(lse, torch.float32, "lse")
    _dense(loss, torch.float32, "loss"), _dense(bad, torch.int32, "bad")
    if target.numel() != R or lse.numel() != R:
        raise RuntimeError(f"{name}: target / lse must hold R = {R} values")
    V, H, bias_arg = _head(E, biased, bias, V)
    ws = _ws("ce", h.device, int(_lib.load().gamer_catalog_ws_bytes(R, V, H, 0)))
    call("gamer_" + name, ptr(h2), h2.stride(0), ptr(idx), idx64, R, ptr(E), V, H, *bias_arg, ptr(target), ptr(lse), ptr(loss),
         ptr(bad), ptr(ws), ws.numel(), stream_ptr())


def _catalog_ce_bwd(biased, h, row_idx, E, bias, target, lse, dloss, scale, dE, dh, dbias, V):
    name = "catalog_ce_bias_bwd" if biased else "catalog_ce_bwd"
    h2, idx, idx64, R = _rows(h, row_idx)
    _dense(E, torch.float32, "E"), _dense(target, torch.int64, "target"), _dense(lse, torch.float32, "lse")
    if dloss is not None:
        _dense(dloss, torch.float32, "dloss")
    if dE is not None and (_dense(dE, torch.float32, "dE").shape != E.shape):
        raise RuntimeError(f"{name}: dE must have E's shape")
    V, H, bias_arg = _head(E, biased, bias, V)
    if dbias is not None and _dense(dbias, torch.float32, "dbias").numel() < V:
        raise RuntimeError(f"{name}: dbias must hold V = {V} values")
    if dh is not None:
        _dense(dh, torch.float32, "dh")                 # (a reshape of a strided dh would be a copy: the writes would be lost)
        if dh.shape[-1] != H or (row_idx is None and dh.numel() // H < R):
            raise RuntimeError(f"{name}: dh must be rows of H values covering the gathered rows")
    dh2 = dh.reshape(-1, dh.shape[-1]) if dh is not None else None
    ws = _ws("ce", h.device, int(_lib.load().gamer_catalog_ws_bytes(R, V, H, 0)))
    call("gamer_" + name, ptr(h2), h2.stride(0), ptr(idx), idx64, R, ptr(E), V, H, *bias_arg, ptr(target), ptr(lse), ptr(dloss),
         float(scale), ptr(dE), ptr(dh2), dh2.stride(0) if dh2 is not None else 0, *((ptr(dbias),) if biased else ()), ptr(ws),
         ws.numel(), stream_ptr())


def _catalog_topk(biased, h, E, bias, k, start, end, row_idx, V):
    h2, idx, idx64, R = _rows(h, row_idx)
    _dense(E, torch.float32, "E")
    V, H, bias_arg = _head(E, biased, bias, V)
    end = V if end is None else int(end)
    ws = _ws("topk", h.device, int(_lib.load().gamer_catalog_ws_bytes(R, max(end - start, 1), H, k)))
    out_i = torch.empty(R, k, dtype=torch.int64, device=h.device)
    out_s = torch.empty(R, k, dtype=torch.float32, device=h.device)
    call("gamer_catalog_topk_bias" if biased else "gamer_catalog_topk", ptr(h2), h2.stride(0), ptr(idx), idx64, R, ptr(E), V, H,
         *bias_arg, int(start), end, int(k), ptr(out_i), ptr(out_s), ptr(ws), ws.numel(), stream_ptr())
    return out_i, out_s


def catalog_ce_fwd(h, row_idx, E, target, lse, loss, bad):
    """lse [R], loss (0-d) = mean CE of the rows h[row_idx] against target over the whole table E (gamer_catalog_ce_fwd)."""
    _catalog_ce_fwd(False, h, row_idx, E, None, target, lse, loss, bad, None)


def catalog_ce_bwd(h, row_idx, E, target, lse, dloss, scale, dE=None, dh=None):
    """dE += G^T h, dh rows (at row_idx of dh's row view) <- G E, G = (softmax - onehot) * dloss * scale (gamer_catalog_ce_bwd)."""
    _catalog_ce_bwd(False, h, row_idx, E, None, target, lse, dloss, scale, dE, dh, None, None)


def catalog_topk(h, E, k, start=0, end=None, row_idx=None):
    """(indices int64 [R, k], scores [R, k]): the k best items of [start, end) per row, ties to the lower index, -1 past the range."""
    return _catalog_topk(False, h, E, None, k, start, end, row_idx, None)


def catalog_ce_bias_fwd(h, row_idx, E, bias, target, lse, loss, bad, V=None):
    """catalog_ce_fwd with score(r, v) = h_r . E_v + bias[v] over the first V rows of E (gamer_catalog_ce_bias_fwd);
    bias None: the same kernels and bits as catalog_ce_fwd."""
    _catalog_ce_fwd(True, h, row_idx, E, bias, target, lse, loss, bad, V)


def catalog_ce_bias_bwd(h, row_idx, E, bias, target, lse, dloss, scale, dE=None, dh=None, dbias=None, V=None):
    """catalog_ce_bwd with the bias in the scores; dE rows [0, V) += G^T h, dh <- G E, dbias [V] <- the column sums of G (written)."""
    _catalog_ce_bwd(True, h, row_idx, E, bias, target, lse, dloss, scale, dE, dh, dbias, V)


def catalog_topk_bias(h, E, bias, k, start=0, end=None, row_idx=None, V=None):
    """catalog_topk with score(r, v) = h_r . E_v + bias[v], over [start, end) of the first V rows of E (gamer_catalog_topk_bias)."""
    return _catalog_topk(True, h, E, bias, k, start, end, row_idx, V)


def cloze_threshold(ratio: float) -> int:
    """the 32-bit threshold gamer_cloze_mask compares a word against: word < threshold (a ratio >= 1 is always true)"""
    t = float(torch.tensor(float(ratio), dtype=torch.float32)) * 4294967296.0
    return 0xFFFFFFFF if t >= 4294967040.0 else max(int(t), 0)


def cloze_mask(ids, seq_len, mask_ratio, ft_ratio, mask_token, max_seq_length, seed, want_words=False):
    """BERT4Rec's cloze masking (gamer_cloze_mask): (masked [B, L], labels [B, L], rows [B L], targets [B L], count [1] int32[,
    words [B L + B]]).  rows / targets hold count[0] entries: the flat positions with labels != 0 in row-major order and their
    labels.  The caller checks seq_len against L and max_seq_length (a position outside the row is ignored here)."""
    _dense(ids, torch.int64, "ids"), _dense(seq_len, torch.int64, "seq_len")
    if ids.dim() != 2 or seq_len.shape != (ids.shape[0],):
        raise RuntimeError("cloze_mask: ids [B, L] and seq_len [B]")
    B, L = ids.shape
    dev = ids.device
    masked, labels = torch.empty_like(ids), torch.empty_like(ids)
    rows = torch.empty(B * L, dtype=torch.int64, device=dev)
    targets = torch.empty(B * L, dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    words = torch.empty(B * L + B, dtype=torch.int64, device=dev) if want_words else None
    ws = _ws("cloze", dev, int(_lib.load().gamer_cloze_mask_ws_bytes(B, L)))
    call("gamer_cloze_mask", ptr(ids), ptr(seq_len), B, L, float(mask_ratio), float(ft_ratio), int(mask_token), int(max_seq_length),
         int(seed), ptr(masked), ptr(labels), ptr(rows), ptr(targets), ptr(count), ptr(words), ptr(ws), ws.numel(), stream_ptr())
    out = (masked, labels, rows, targets, count)
    return out + (words,) if want_words else out


def embedding_bwd_large(ids, dx, pad_id, dW):
    """dW[id] += dx rows in token order, pad_id skipped, any table size (gamer_embedding_bwd_large)."""
    _dense(ids, torch.int64, "ids"), _dense(dx, torch.float32, "dx"), _dense(dW, torch.float32, "dW")
    T = ids.numel()
    V, H = dW.shape
    if dx.numel() != T * H:
        raise RuntimeError("embedding_bwd_large: dx must hold one row of H values per id")
    ws = _ws("emb_large", dx.device, int(_lib.load().gamer_embedding_bwd_large_ws_bytes(V, T, H)))
    call("gamer_embedding_bwd_large", ptr(ids), ptr(dx), V, T, H, pad_id, ptr(dW), ptr(ws), ws.numel(), stream_ptr())


def position_bwd(dx, dP):
    """dP [S, H] += dx [B, S, H] summed over the batch in order (gamer_position_bwd)."""
    _dense(dx, torch.float32, "dx"), _dense(dP, torch.float32, "dP")
    B, S, H = dx.shape
    if dP.shape != (S, H):
        raise RuntimeError(f"position_bwd: dP must be [{S}, {H}]")
    nf = int(_lib.load().gamer_position_bwd_ws_floats(B, S, H))
    ws = _ws("pos", dx.device, 4 * nf)
    call("gamer_position_bwd", ptr(dx), B, S, H, ptr(dP), ptr(ws), nf, stream_ptr())


def seq_embed_ln_fwd(ids, E, P, w, b, eps, p, seed, v, y, mean, rstd):
    """y = dropout(LayerNorm(E[ids] + P[s])) for ids [B, S] (gamer_seq_embed_ln_fwd); v / mean / rstd for the backward."""
    _dense(ids, torch.int64, "ids")
    for t, n in ((E, "E"), (P, "P"), (w, "w"), (b, "b"), (v, "v"), (y, "y"), (mean, "mean"), (rstd, "rstd")):
        _dense(t, torch.float32, n)
    B, S = ids.shape
    V, H = E.shape
    if P.shape[0] < S or P.shape[1] != H:
        raise RuntimeError(f"seq_embed_ln_fwd: the position table must have >= {S} rows of {H}")
    call("gamer_seq_embed_ln_fwd", ptr(ids), ptr(E), V, ptr(P), B, S, H, ptr(w), ptr(b), float(eps), float(p), int(seed), ptr(v), ptr(y),
         ptr(mean), ptr(rstd), stream_ptr())


# ---- GRU recurrence of GRU4Rec (csrc/gru.hip) ----------------------------------------------------------------------------------
def _gru_check(B, L, H, lens):
    if not (B >= 1 and L >= 1 and 16 <= H <= 256 and H % 16 == 0):
        raise RuntimeError(f"gru: B={B} L={L} H={H} (B, L >= 1; H % 16 == 0, 16 <= H <= 256)")
    if lens is not None:
        _dense(lens, torch.int64, "lens")
        if lens.numel() != B:
            raise RuntimeError(f"gru: lens must hold B = {B} values")
    return ptr(lens) if lens is not None else None


def gru_gates_floats(B, L, H):
    return int(_lib.load().gamer_gru_gates_floats(B, L, H))


def gru_fwd(gi, w_hh, h, gates=None, lens=None):
    """h [B, L, H] = the GRU's h_t of every step from gi [B, L, 3H] = x W_ih^T (gamer_gru_fwd); gates [B, L, 4, H] (training)
    keeps r, z, n and W_hn h_{t-1} for gru_bwd."""
    _dense(gi, torch.float32, "gi"), _dense(w_hh, torch.float32, "w_hh"), _dense(h, torch.float32, "h")
    B, L, H = h.shape
    lp = _gru_check(B, L, H, lens)
    if gi.shape != (B, L, 3 * H) or w_hh.shape != (3 * H, H):
        raise RuntimeError(f"gru_fwd: gi must be [{B}, {L}, {3 * H}] and w_hh [{3 * H}, {H}]")
    if gates is not None and (_dense(gates, torch.float32, "gates").numel() != gru_gates_floats(B, L, H)):
        raise RuntimeError(f"gru_fwd: gates must hold {gru_gates_floats(B, L, H)} floats")
    call("gamer_gru_fwd", ptr(gi), ptr(w_hh), lp, B, L, H, ptr(h), ptr(gates), stream_ptr())


def gru_bwd(dy, h, gates, w_hh, dgi, dgh_next, lens=None):
    """dgi, dgh_next [B, L, 3H] from the upstream gradient dy [B, L, H] of every h_t (gamer_gru_bwd): dW_ih = dgi^T x,
    dW_hh = dgh_next^T h, dx = dgi W_ih."""
    for t, n in ((dy, "dy"), (h, "h"), (gates, "gates"), (w_hh, "w_hh"), (dgi, "dgi"), (dgh_next, "dgh_next")):
        _dense(t, torch.float32, n)
    B, L, H = h.shape
    lp = _gru_check(B, L, H, lens)
    if dy.shape != h.shape or w_hh.shape != (3 * H, H) or dgi.shape != (B, L, 3 * H) or dgh_next.shape != (B, L, 3 * H):
        raise RuntimeError(f"gru_bwd: dy [{B}, {L}, {H}], w_hh [{3 * H}, {H}], dgi / dgh_next [{B}, {L}, {3 * H}]")
    if gates.numel() != gru_gates_floats(B, L, H):
        raise RuntimeError(f"gru_bwd: gates must hold {gru_gates_floats(B, L, H)} floats")
    call("gamer_gru_bwd", ptr(dy), ptr(h), ptr(gates), ptr(w_hh), lp, B, L, H, ptr(dgi), ptr(dgh_next), stream_ptr())


# ---- MBSTR's behaviour-aware attention and CGC head (csrc/mbs_attention.hip) -----------------------------------------------------
MBS_MAX_L, MBS_MAX_D, MBS_MAX_B, MBS_MAX_E = 128, 64, 8, 16


def mbs_check_limits(L, H, d, b):
    """The limits of the MBSTR kernels, refused on the host before any launch."""
    if L > MBS_MAX_L or d > MBS_MAX_D or H > 256 or H % 4 or b > MBS_MAX_B or L < 1 or b < 1:
        raise NotImplementedError(f"MBSTR on the HIP path: L <= {MBS_MAX_L}, head size <= {MBS_MAX_D}, hidden size <= 256 and "
                                  f"divisible by 4, n_behaviors <= {MBS_MAX_B} (got L={L}, head size={d}, hidden size={H}, "
                                  f"n_behaviors={b})")


def mbs_mix_fwd(W, alpha, Wm):
    """Wm [b b + 1, h, d, d] = sum_j softmax_j(alpha [b b + 1, b, h]) W [b, h, d, d] (gamer_mbs_mix_fwd)."""
    for t, n in ((W, "W"), (alpha, "alpha"), (Wm, "Wm")):
        _dense(t, torch.float32, n)
    b, h, d, _ = W.shape
    if alpha.shape != (b * b + 1, b, h) or Wm.shape != (b * b + 1, h, d, d):
        raise RuntimeError(f"mbs_mix_fwd: alpha [{b * b + 1}, {b}, {h}] and Wm [{b * b + 1}, {h}, {d}, {d}]")
    call("gamer_mbs_mix_fwd", ptr(W), ptr(alpha), b, h, d, ptr(Wm), stream_ptr())


def mbs_mix_bwd(W, alpha, dWm, dW, dalpha):
    for t, n in ((W, "W"), (alpha, "alpha"), (dWm, "dWm"), (dW, "dW"), (dalpha, "dalpha")):
        _dense(t, torch.float32, n)
    b, h, d, _ = W.shape
    if alpha.shape != (b * b + 1, b, h) or dWm.shape != (b * b + 1, h, d, d) or dW.shape != W.shape or dalpha.shape != alpha.shape:
        raise RuntimeError("mbs_mix_bwd: shapes of mbs_mix_fwd")
    call("gamer_mbs_mix_bwd", ptr(W), ptr(alpha), ptr(dWm), b, h, d, ptr(dW), ptr(dalpha), stream_ptr())


def _mbs_common(q, k, v, types, w1m, w2m, rel, bucket, B, L, h, d, b):
    mbs_check_limits(L, h * d, d, b)
    C_ = b * b + 1
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        _chk(t, torch.float32, n)
        if t.dim() != 2 or t.shape[0] != B * L or t.shape[1] != h * d or t.stride(1) != 1:
            raise RuntimeError(f"mbs attention: {n} must be a [{B * L}, {h * d}] row-strided view")
    _dense(types, torch.int32, "types"), _dense(w1m, torch.float32, "w1m"), _dense(w2m, torch.float32, "w2m")
    if types.shape != (B, L) or w1m.shape != (C_, h, d, d) or w2m.shape != (C_, h, d, d):
        raise RuntimeError(f"mbs attention: types [{B}, {L}], w1m / w2m [{C_}, {h}, {d}, {d}]")
    nb = 0
    if rel is not None:
        _dense(rel, torch.float32, "rel"), _dense(bucket, torch.int32, "bucket")
        nb = rel.shape[1]
        if rel.shape != (C_, nb, h) or bucket.shape != (2 * L - 1,):
            raise RuntimeError(f"mbs attention: rel [{C_}, num_buckets, {h}] and bucket [{2 * L - 1}]")
    return nb


def mbs_attn_fwd(q, k, v, types, w1m, w2m, rel, bucket, B, L, h, d, b, scale, p_drop, seed, o, lse):
    """gamer_mbs_attn_fwd: q / k / v / o [B L, h d] (row-strided views), types int32 [B, L], rel [b b + 1, num_buckets, h] or None,
    bucket int32 [2 L - 1] (values in [0, num_buckets): checked by the caller), lse [B, h, L]."""
    nb = _mbs_common(q, k, v, types, w1m, w2m, rel, bucket, B, L, h, d, b)
    _chk(o, torch.float32, "o"), _dense(lse, torch.float32, "lse")
    if o.shape != (B * L, h * d) or o.stride(1) != 1 or lse.numel() != B * h * L:
        raise RuntimeError("mbs_attn_fwd: o [B L, h d] and lse [B, h, L]")
    call("gamer_mbs_attn_fwd", ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v), v.stride(0), ptr(types), ptr(w1m), ptr(w2m), ptr(rel),
         ptr(bucket) if rel is not None else None, nb, B, L, h, d, b, float(scale), float(p_drop), int(seed), ptr(o), o.stride(0),
         ptr(lse), stream_ptr())


def mbs_n_partial(B, h, d, b):
    """Slabs of the attention backward's parameter gradients: n h workgroups, one per CU (256) when the slab sets allow it - at
    most 24 MB each (two of them, W1m's and W2m's)."""
    n = max(1, min(B, 256 // max(1, h)))
    while n > 1 and n * (b * b + 1) * h * d * d * 4 > (24 << 20):
        n //= 2
    return n


def mbs_attn_bwd(q, k, v, types, w1m, w2m, rel, bucket, B, L, h, d, b, scale, p_drop, seed, o, d_o, lse, dq, dk, dv, dw1m_partial,
                 dw2m_partial, drel_partial):
    """gamer_mbs_attn_bwd: dq / dk / dv and the three partial slab sets must be zero on entry; dw*_partial [n, b b + 1, h, d, d],
    drel_partial [n, b b + 1, 2 L - 1, h] (None iff rel is None)."""
    nb = _mbs_common(q, k, v, types, w1m, w2m, rel, bucket, B, L, h, d, b)
    C_ = b * b + 1
    for t, n in ((o, "o"), (d_o, "d_o"), (dq, "dq"), (dk, "dk"), (dv, "dv")):
        _chk(t, torch.float32, n)
        if t.shape != (B * L, h * d) or t.stride(1) != 1:
            raise RuntimeError(f"mbs_attn_bwd: {n} must be a [{B * L}, {h * d}] row-strided view")
    if o.stride(0) != d_o.stride(0):
        raise RuntimeError("mbs_attn_bwd: o and d_o must share their row stride")
    _dense(lse, torch.float32, "lse"), _dense(dw1m_partial, torch.float32, "dw1m_partial"), _dense(dw2m_partial, torch.float32, "dw2m_partial")
    n = dw1m_partial.shape[0]
    if dw1m_partial.shape != (n, C_, h, d, d) or dw2m_partial.shape != (n, C_, h, d, d) or lse.numel() != B * h * L:
        raise RuntimeError("mbs_attn_bwd: partial slabs [n, b b + 1, h, d, d], lse [B, h, L]")
    if (rel is None) != (drel_partial is None):
        raise RuntimeError("mbs_attn_bwd: drel_partial goes with the bias table")
    if drel_partial is not None and (_dense(drel_partial, torch.float32, "drel_partial").shape != (n, C_, 2 * L - 1, h)):
        raise RuntimeError(f"mbs_attn_bwd: drel_partial [{n}, {C_}, {2 * L - 1}, {h}]")
    call("gamer_mbs_attn_bwd", ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v), v.stride(0), ptr(types), ptr(w1m), ptr(w2m), ptr(rel),
         ptr(bucket) if rel is not None else None, nb, B, L, h, d, b, float(scale), float(p_drop), int(seed), ptr(o), ptr(d_o),
         o.stride(0), ptr(lse), ptr(dq), dq.stride(0), ptr(dk), dk.stride(0), ptr(dv), dv.stride(0), ptr(dw1m_partial),
         ptr(dw2m_partial), ptr(drel_partial), n, stream_ptr())


def mbs_bias_fold(drel, bucket, dbias):
    """dbias [C, num_buckets, h] from the per-offset sums drel [C, 2 L - 1, h] (gamer_mbs_bias_fold)."""
    _dense(drel, torch.float32, "drel"), _dense(bucket, torch.int32, "bucket"), _dense(dbias, torch.float32, "dbias")
    C_, R, h = drel.shape
    if bucket.shape != (R,) or dbias.shape[0] != C_ or dbias.shape[2] != h:
        raise RuntimeError("mbs_bias_fold: drel [C, 2 L - 1, h], bucket [2 L - 1], dbias [C, num_buckets, h]")
    call("gamer_mbs_bias_fold", ptr(drel), ptr(bucket), (R + 1) // 2, C_, dbias.shape[1], h, ptr(dbias), stream_ptr())


def mbs_gate_mix_fwd(logits, outs, types, gates, mix):
    """gates [M, E] = softmax(logits [M, >= E][:, :E]); mix [M, H] = sum_e gates_e outs [M, E, H]; rows of type 0: zeros."""
    _chk(logits, torch.float32, "logits"), _dense(outs, torch.float32, "outs"), _dense(types, torch.int32, "types")
    _dense(gates, torch.float32, "gates"), _dense(mix, torch.float32, "mix")
    M, E, H = outs.shape
    if E > MBS_MAX_E or logits.shape[0] != M or logits.shape[1] < E or logits.stride(1) != 1 or types.shape != (M,) or gates.shape != (M, E) \
            or mix.shape != (M, H):
        raise RuntimeError(f"mbs_gate_mix_fwd: bad shapes (E <= {MBS_MAX_E})")
    call("gamer_mbs_gate_mix_fwd", ptr(logits), logits.stride(0), ptr(outs), ptr(types), M, E, H, ptr(gates), ptr(mix), stream_ptr())


def mbs_gate_mix_bwd(gates, outs, dmix, douts, dlogits):
    for t, n in ((gates, "gates"), (outs, "outs"), (dmix, "dmix"), (douts, "douts")):
        _dense(t, torch.float32, n)
    _chk(dlogits, torch.float32, "dlogits")
    M, E, H = outs.shape
    if gates.shape != (M, E) or dmix.shape != (M, H) or douts.shape != outs.shape or dlogits.shape[0] != M or dlogits.shape[1] < E \
            or dlogits.stride(1) != 1:
        raise RuntimeError("mbs_gate_mix_bwd: bad shapes")
    call("gamer_mbs_gate_mix_bwd", ptr(gates), ptr(outs), ptr(dmix), M, E, H, ptr(douts), ptr(dlogits), dlogits.stride(0), stream_ptr())


# ---- residual quantiser of the RQ-VAE item tokenizer (csrc/rqvae.hip) ------------------------------------------------------------
RVQ_MAX_LEVELS, RVQ_MAX_D, RVQ_MAX_K = 8, 64, 1024


def rvq_check_limits(num_emb_list, e_dim):
    """The limits of the quantiser kernels as the module reports them (the entry points refuse them too, before any launch)."""
    if not (1 <= len(num_emb_list) <= RVQ_MAX_LEVELS and all(1 <= k <= RVQ_MAX_K for k in num_emb_list)
            and 4 <= e_dim <= RVQ_MAX_D and e_dim % 4 == 0):
        raise NotImplementedError(f"RQ-VAE on the HIP path: at most {RVQ_MAX_LEVELS} levels of at most {RVQ_MAX_K} codes, e_dim a "
                                  f"multiple of 4 and at most {RVQ_MAX_D} (got num_emb_list={list(num_emb_list)}, e_dim={e_dim})")


def _i32_array(values):
    return (C.c_int32 * len(values))(*[int(v) for v in values])


def rvq_ws_floats(B):
    return int(_lib.load().gamer_rvq_ws_floats(B))


def rvq_fwd(r, codebooks, level_offsets, modes, level_begin, level_end, idx, x_q, residual, r_levels=None, dist=None,
            loss_sums=None):
    """Levels [level_begin, level_end) of the residual quantiser on r [B, D] (rows may be strided; gamer_rvq_fwd).  level_offsets /
    modes: Python sequences (n_levels + 1 / n_levels values).  idx int32 [B, n_levels]; x_q, residual [B, D]; r_levels
    [n_levels, B, D]; dist [B, K of level_end - 1] makes that level distance-only; loss_sums [n_levels]."""
    n_levels = len(modes)
    B, D = (r.shape[0], r.shape[1]) if r is not None else (x_q.shape[0], x_q.shape[1])
    ws = None
    if loss_sums is not None:
        ws = _ws("rvq", loss_sums.device, 4 * max(rvq_ws_floats(B), 1))
    ldr = r.stride(0) if r is not None else D
    call("gamer_rvq_fwd", ptr(r), ldr, ptr(codebooks), _i32_array(level_offsets), _i32_array(modes), n_levels, level_begin,
         level_end, B, D, ptr(idx), ptr(x_q), ptr(residual), ptr(r_levels), ptr(dist), ptr(ws), ptr(loss_sums), stream_ptr())


def rvq_bwd(idx, r_levels, codebooks, level_offsets, g_xq, g_level, mu, dz, dE):
    """dz [B, D] and dE [sum K, D] of the quantiser losses (gamer_rvq_bwd): g_xq [B, D] or None, g_level [n_levels] on the device."""
    n_levels = len(level_offsets) - 1
    B, D = dz.shape
    call("gamer_rvq_bwd", ptr(idx), ptr(r_levels), ptr(codebooks), _i32_array(level_offsets), n_levels, B, D, ptr(g_xq),
         ptr(g_level), float(mu), ptr(dz), ptr(dE), stream_ptr())


# ---- MBHT's multi-scale encoder layer (csrc/mbht.hip) ---------------------------------------------------------------------------
MBHT_MAX_L, MBHT_MAX_D, MBHT_MAX_H, MBHT_MAX_C, MBHT_MAX_HYPER = 128, 64, 256, 16, 8


def mbht_check_limits(L, H, d, c=1, hyper_len=1):
    """The limits of the MBHT kernels, refused on the host before any launch."""
    if L > MBHT_MAX_L or d > MBHT_MAX_D or H > MBHT_MAX_H or H % 4 or c > MBHT_MAX_C or hyper_len > MBHT_MAX_HYPER or min(L, c, hyper_len) < 1:
        raise NotImplementedError(f"MBHT on the HIP path: L <= {MBHT_MAX_L}, head size <= {MBHT_MAX_D}, hidden size <= {MBHT_MAX_H} "
                                  f"and divisible by 4, scales[0] <= {MBHT_MAX_C}, hyper_len <= {MBHT_MAX_HYPER} (got L={L}, head "
                                  f"size={d}, hidden size={H}, scales[0]={c}, hyper_len={hyper_len})")


def _msa_common(q, k, v, keep, Ew, Eb, Fw, Fb, B, L, h, d):
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        _chk(t, torch.float32, n)
        if t.dim() != 2 or t.shape[0] != B * L or t.shape[1] != h * d or t.stride(1) != 1:
            raise RuntimeError(f"msa linear attention: {n} must be a [{B * L}, {h * d}] row-strided view")
    _dense(keep, torch.int32, "keep")
    for t, n in ((Ew, "Ew"), (Eb, "Eb"), (Fw, "Fw"), (Fb, "Fb")):
        _dense(t, torch.float32, n)
    c = Ew.shape[0]
    mbht_check_limits(L, h * d, d, c)
    if keep.shape != (B, L) or Ew.shape != (c, L) or Fw.shape != (c, L) or Eb.shape != (c,) or Fb.shape != (c,):
        raise RuntimeError(f"msa linear attention: keep [{B}, {L}], Ew / Fw [c, {L}], Eb / Fb [c]")
    return c


def msa_linear_fwd(q, k, v, keep, Ew, Eb, Fw, Fb, B, L, h, d, scale, p_drop, seed, o, lse):
    """gamer_msa_linear_fwd: q / k / v / o [B L, h d] (row-strided views), keep int32 [B, L], Ew / Fw [c, L] (the projections of
    the values / the keys), lse [B, h, L]."""
    c = _msa_common(q, k, v, keep, Ew, Eb, Fw, Fb, B, L, h, d)
    _chk(o, torch.float32, "o"), _dense(lse, torch.float32, "lse")
    if o.shape != (B * L, h * d) or o.stride(1) != 1 or lse.numel() != B * h * L:
        raise RuntimeError("msa_linear_fwd: o [B L, h d] and lse [B, h, L]")
    call("gamer_msa_linear_fwd", ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v), v.stride(0), ptr(keep), ptr(Ew), ptr(Eb), ptr(Fw),
         ptr(Fb), B, L, h, d, c, float(scale), float(p_drop), int(seed), ptr(o), o.stride(0), ptr(lse), stream_ptr())


def msa_n_partial(B, h):
    """slabs of the linear attention's backward: one workgroup per CU (256) at the most"""
    return max(1, min(B * h, 256))


def msa_linear_bwd(q, k, v, keep, Ew, Eb, Fw, Fb, B, L, h, d, scale, p_drop, seed, d_o, lse, dq, dk, dv, partial):
    """gamer_msa_linear_bwd: dq / dk / dv are written; partial [n, 2 c L + 2 c] must be zero on entry; its column sums are
    [dEw | dFw | dEb | dFb]."""
    c = _msa_common(q, k, v, keep, Ew, Eb, Fw, Fb, B, L, h, d)
    for t, n in ((d_o, "d_o"), (dq, "dq"), (dk, "dk"), (dv, "dv")):
        _chk(t, torch.float32, n)
        if t.shape != (B * L, h * d) or t.stride(1) != 1:
            raise RuntimeError(f"msa_linear_bwd: {n} must be a [{B * L}, {h * d}] row-strided view")
    _dense(lse, torch.float32, "lse"), _dense(partial, torch.float32, "partial")
    n = partial.shape[0]
    if partial.shape != (n, 2 * c * L + 2 * c) or not 1 <= n <= B * h or lse.numel() != B * h * L:
        raise RuntimeError(f"msa_linear_bwd: partial [n <= {B * h}, {2 * c * L + 2 * c}], lse [B, h, L]")
    call("gamer_msa_linear_bwd", ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v), v.stride(0), ptr(keep), ptr(Ew), ptr(Eb), ptr(Fw),
         ptr(Fb), B, L, h, d, c, float(scale), float(p_drop), int(seed), ptr(d_o), d_o.stride(0), ptr(lse), ptr(dq), dq.stride(0),
         ptr(dk), dk.stride(0), ptr(dv), dv.stride(0), ptr(partial), n, stream_ptr())


def _seq_mix_common(xs, W, B, H, what):
    if not 1 <= len(xs) <= 3:
        raise RuntimeError(f"{what}: one to three sources")
    lens = []
    for i, x in enumerate(xs):
        _dense(x, torch.float32, f"x{i}")
        if x.dim() != 3 or x.shape[0] != B or x.shape[2] != H or x.shape[1] < 1:
            raise RuntimeError(f"{what}: x{i} must be [{B}, L{i}, {H}]")
        lens.append(x.shape[1])
    _dense(W, torch.float32, "W")
    if W.dim() != 2 or W.shape[1] != sum(lens):
        raise RuntimeError(f"{what}: W [Lout, {sum(lens)}]")
    Lout = W.shape[0]
    if H > MBHT_MAX_H or max(lens + [Lout]) > MBHT_MAX_L:
        raise NotImplementedError(f"{what}: hidden size <= {MBHT_MAX_H}, every length <= {MBHT_MAX_L}")
    return lens + [0] * (3 - len(xs)), Lout


def seq_mix_fwd(xs, W, bias, y):
    """y [B, Lout, H] = W [Lout, sum L_i] cat(xs, 1) + bias[:, None] (gamer_seq_mix_fwd); xs: one to three [B, L_i, H]."""
    B, Lout_, H = y.shape
    lens, Lout = _seq_mix_common(xs, W, B, H, "seq_mix_fwd")
    _dense(bias, torch.float32, "bias"), _dense(y, torch.float32, "y")
    if Lout_ != Lout or bias.shape != (Lout,):
        raise RuntimeError(f"seq_mix_fwd: y [{B}, {Lout}, {H}] and bias [{Lout}]")
    px = [ptr(x) for x in xs] + [None] * (3 - len(xs))
    call("gamer_seq_mix_fwd", px[0], lens[0], px[1], lens[1], px[2], lens[2], ptr(W), ptr(bias), B, H, Lout, ptr(y), stream_ptr())


def seq_mix_n_partial(B, Lout, Lin):
    """slabs of seq_mix_bwd: one workgroup per CU (256) when the slabs stay below 32 MB"""
    n = max(1, min(B, 256))
    while n > 1 and n * (Lout * Lin + Lout) * 4 > (32 << 20):
        n //= 2
    return n


def seq_mix_bwd(xs, W, dy, dxs, partial):
    """gamer_seq_mix_bwd: dxs (shapes of xs) are written; partial [n, Lout Lin + Lout] must be zero on entry; its column sums are
    [dW | dbias]."""
    B, Lout_, H = dy.shape
    lens, Lout = _seq_mix_common(xs, W, B, H, "seq_mix_bwd")
    _dense(dy, torch.float32, "dy"), _dense(partial, torch.float32, "partial")
    if len(dxs) != len(xs) or any(_dense(d, torch.float32, "dx").shape != x.shape for d, x in zip(dxs, xs)) or Lout_ != Lout:
        raise RuntimeError("seq_mix_bwd: dy [B, Lout, H] and one dx per source, of its shape")
    n = partial.shape[0]
    if partial.shape != (n, Lout * sum(lens) + Lout) or not 1 <= n <= B:
        raise RuntimeError(f"seq_mix_bwd: partial [n <= {B}, {Lout * sum(lens) + Lout}]")
    px = [ptr(x) for x in xs] + [None] * (3 - len(xs))
    pd = [ptr(d) for d in dxs] + [None] * (3 - len(xs))
    call("gamer_seq_mix_bwd", px[0], lens[0], px[1], lens[1], px[2], lens[2], ptr(W), ptr(dy), B, H, Lout, pd[0], pd[1], pd[2],
         ptr(partial), n, stream_ptr())


def _hg_check(x, B, L, H, name):
    _dense(x, torch.float32, name)
    if x.shape != (B, L, H):
        raise RuntimeError(f"{name} must be [{B}, {L}, {H}]")


def hg_build_fwd(xm, items, mask_token, hyper_len, G, sel):
    """gamer_hg_build_fwd: xm [B, L, H], items int32 [B, L] (right-padded with 0) -> G [B, L, L] (zero outside the live block) and
    sel int32 [B, L, hyper_len] (the selected key positions of every live row that is no <MASK>, best first; -1 unused)."""
    B, L, H = xm.shape
    mbht_check_limits(L, H, 1, 1, hyper_len)
    _hg_check(xm, B, L, H, "xm"), _dense(items, torch.int32, "items"), _dense(G, torch.float32, "G"), _dense(sel, torch.int32, "sel")
    if items.shape != (B, L) or G.shape != (B, L, L) or sel.shape != (B, L, hyper_len):
        raise RuntimeError(f"hg_build_fwd: items [{B}, {L}], G [{B}, {L}, {L}], sel [{B}, {L}, {hyper_len}]")
    call("gamer_hg_build_fwd", ptr(xm), ptr(items), B, L, H, hyper_len, int(mask_token), ptr(G), ptr(sel), stream_ptr())


def hg_build_bwd(xm, items, sel, G, dG, mask_token, dxm):
    """gamer_hg_build_bwd: dxm [B, L, H] from dG [B, L, L] along the selection ``sel`` of the forward."""
    B, L, H = xm.shape
    K = sel.shape[-1]
    mbht_check_limits(L, H, 1, 1, K)
    _hg_check(xm, B, L, H, "xm"), _hg_check(dxm, B, L, H, "dxm"), _dense(items, torch.int32, "items"), _dense(sel, torch.int32, "sel")
    _dense(G, torch.float32, "G"), _dense(dG, torch.float32, "dG")
    if items.shape != (B, L) or G.shape != (B, L, L) or dG.shape != (B, L, L) or sel.shape != (B, L, K):
        raise RuntimeError(f"hg_build_bwd: items [{B}, {L}], G / dG [{B}, {L}, {L}], sel [{B}, {L}, K]")
    call("gamer_hg_build_bwd", ptr(xm), ptr(items), ptr(sel), ptr(G), ptr(dG), B, L, H, K, int(mask_token), ptr(dxm), stream_ptr())


def hg_conv_fwd(G, x, y):
    """y [B, L, H] = G [B, L, L] x [B, L, H], row by row of the batch (gamer_hg_conv_fwd)."""
    B, L, H = x.shape
    mbht_check_limits(L, H, 1)
    _hg_check(x, B, L, H, "x"), _hg_check(y, B, L, H, "y"), _hg_check(G, B, L, L, "G")
    call("gamer_hg_conv_fwd", ptr(G), ptr(x), B, L, H, ptr(y), stream_ptr())


def hg_conv_bwd(G, x, dy, dx, dG):
    """dx = G^T dy and dG = dy x^T (gamer_hg_conv_bwd)."""
    B, L, H = x.shape
    mbht_check_limits(L, H, 1)
    _hg_check(x, B, L, H, "x"), _hg_check(dy, B, L, H, "dy"), _hg_check(dx, B, L, H, "dx"), _hg_check(G, B, L, L, "G"), _hg_check(dG, B, L, L, "dG")
    call("gamer_hg_conv_bwd", ptr(G), ptr(x), ptr(dy), B, L, H, ptr(dx), ptr(dG), stream_ptr())


def _hg_readout(name, a, pos, n_obj, out, before, follow, evaluation):
    B, L, H = a.shape
    mbht_check_limits(L, H, 1)
    _hg_check(a, B, L, H, "x"), _hg_check(out, B, L, H, "out"), _dense(pos, torch.int32, "pos"), _dense(n_obj, torch.int32, "n_obj")
    if pos.dim() != 2 or pos.shape[0] != B or pos.shape[1] < 1 or n_obj.shape != (B,):
        raise RuntimeError(f"{name}: pos [{B}, P] and n_obj [{B}]")
    call(name, ptr(a), ptr(pos), ptr(n_obj), B, L, H, pos.shape[1], int(before), int(follow), 1 if evaluation else 0, ptr(out), stream_ptr())


def hg_readout_fwd(x, pos, n_obj, out, before=10, follow=6, evaluation=False):
    """gamer_hg_readout_fwd: out = x with the rows pos[b] (int32 [B, P], in order; training: entries <= 0 skipped) replaced, one
    after the other, by the mean of their sliding window; n_obj int32 [B] = the live positions of each row."""
    _hg_readout("gamer_hg_readout_fwd", x, pos, n_obj, out, before, follow, evaluation)


def hg_readout_bwd(dout, pos, n_obj, dx, before=10, follow=6, evaluation=False):
    _hg_readout("gamer_hg_readout_bwd", dout, pos, n_obj, dx, before, follow, evaluation)


def hg_fuse_fwd(x0, x1, w, out, p0):
    """out [T, H] = p0 x0 + (1 - p0) x1 with p0 [T] = softmax over the two sources of x_s . w (gamer_hg_fuse_fwd)."""
    T, H = x0.shape
    for t, n in ((x0, "x0"), (x1, "x1"), (out, "out")):
        if _dense(t, torch.float32, n).shape != (T, H):
            raise RuntimeError(f"hg_fuse_fwd: {n} must be [{T}, {H}]")
    if _dense(w, torch.float32, "w").shape != (H,) or _dense(p0, torch.float32, "p0").shape != (T,) or H > MBHT_MAX_H:
        raise RuntimeError(f"hg_fuse_fwd: w [{H}], p0 [{T}], H <= {MBHT_MAX_H}")
    call("gamer_hg_fuse_fwd", ptr(x0), ptr(x1), ptr(w), T, H, ptr(out), ptr(p0), stream_ptr())


def hg_fuse_bwd(x0, x1, w, p0, dout, dx0, dx1, partial):
    """gamer_hg_fuse_bwd: dx0 / dx1 are written; partial [n, H] is written, its column sums are dw."""
    T, H = x0.shape
    for t, n in ((x0, "x0"), (x1, "x1"), (dout, "dout"), (dx0, "dx0"), (dx1, "dx1")):
        if _dense(t, torch.float32, n).shape != (T, H):
            raise RuntimeError(f"hg_fuse_bwd: {n} must be [{T}, {H}]")
    _dense(partial, torch.float32, "partial")
    if _dense(w, torch.float32, "w").shape != (H,) or _dense(p0, torch.float32, "p0").shape != (T,) or partial.dim() != 2 or \
            partial.shape[1] != H or H > MBHT_MAX_H:
        raise RuntimeError(f"hg_fuse_bwd: w [{H}], p0 [{T}], partial [n, {H}], H <= {MBHT_MAX_H}")
    call("gamer_hg_fuse_bwd", ptr(x0), ptr(x1), ptr(w), ptr(p0), ptr(dout), T, H, ptr(dx0), ptr(dx1), ptr(partial), partial.shape[0],
         stream_ptr())


# ---- PBAT's fused Wasserstein attention and head (csrc/pbat.hip) ------------------------------------------------------------------
PBAT_MAX_L, PBAT_MAX_D, PBAT_MAX_B, PBAT_MAX_H = 128, 64, 8, 128


def pbat_check_limits(L, H, d, b):
    """The limits of the PBAT kernels, refused on the host before any launch (hidden size: the head runs the biased catalogue
    kernels at 2 H <= 256)."""
    if L > PBAT_MAX_L or L < 1 or d > PBAT_MAX_D or d % 4 or H > PBAT_MAX_H or H % 4 or b > PBAT_MAX_B or b < 1:
        raise NotImplementedError(f"PBAT on the HIP path: L <= {PBAT_MAX_L}, head size <= {PBAT_MAX_D} and a multiple of 4, hidden "
                                  f"size <= {PBAT_MAX_H} and a multiple of 4, n_behaviors <= {PBAT_MAX_B} (got L={L}, head size={d}, "
                                  f"hidden size={H}, n_behaviors={b})")


def _pbat_common(name, proj, rel_m, rel_c, pos_m, pos_c, weights, types, keep, B, L, h, d, b):
    pbat_check_limits(L, h * d, d, b)
    H, NP = h * d, (b + 1) * (b + 1)
    if len(proj) != 6 or len(weights) != 8:
        raise RuntimeError(f"{name}: six projections (q1, q2, k1, k2, v1, v2) and (Wq1, bq1, Wq2, bq2, Wk1, bk1, Wk2, bk2)")
    for t in proj:
        _chk(t, torch.float32, "projection")
        if t.shape != (B * L, H) or t.stride(1) != 1 or t.stride(0) != proj[0].stride(0):
            raise RuntimeError(f"{name}: the projections must be [{B * L}, {H}] row-strided views with one row stride")
    for t, n, shp in ((rel_m, "rel_m", (B, NP, H)), (rel_c, "rel_c", (B, NP, H)), (pos_m, "pos_m", (L, H)), (pos_c, "pos_c", (L, H))):
        if _dense(t, torch.float32, n).shape != shp:
            raise RuntimeError(f"{name}: {n} must be {list(shp)}")
    for i, w in enumerate(weights):
        if _dense(w, torch.float32, "weight").shape != ((d,) if i % 2 else (d, d)):
            raise RuntimeError(f"{name}: Wq1 / Wq2 / Wk1 / Wk2 [{d}, {d}] with biases [{d}]")
    if _dense(types, torch.int32, "types").shape != (B, L) or _dense(keep, torch.int32, "keep").shape != (B, L):
        raise RuntimeError(f"{name}: types / keep int32 [{B}, {L}]")
    ws = _ws("pbat_pos", proj[0].device, 2 * H * L * 4)
    return ([ptr(t) for t in proj] + [proj[0].stride(0), ptr(rel_m), ptr(rel_c), ptr(pos_m), ptr(pos_c)] + [ptr(w) for w in weights]
            + [ptr(types), ptr(keep), B, L, h, d, b]), ws


def pbat_attn_fwd(proj, rel_m, rel_c, pos_m, pos_c, weights, types, keep, B, L, h, d, b, scale, p_drop, seed, o1, o2, S, lse):
    """gamer_pbat_attn_fwd: proj = (q1, q2, k1, k2, v1, v2) [B L, h d] row-strided views; rel_m / rel_c [B, (b + 1)^2, h d]; pos_m /
    pos_c [L, h d]; weights = (Wq1, bq1, Wq2, bq2, Wk1, bk1, Wk2, bk2); types / keep int32 [B, L]; o1 / o2 [B L, h d]; S [B, h, L,
    b + 1] and lse [B, h, L] are what the backward needs."""
    args, ws = _pbat_common("pbat_attn_fwd", proj, rel_m, rel_c, pos_m, pos_c, weights, types, keep, B, L, h, d, b)
    for t in (o1, o2):
        _chk(t, torch.float32, "o")
        if t.shape != (B * L, h * d) or t.stride(1) != 1 or t.stride(0) != o1.stride(0):
            raise RuntimeError("pbat_attn_fwd: o1 / o2 [B L, h d] with one row stride")
    if _dense(S, torch.float32, "S").shape != (B, h, L, b + 1) or _dense(lse, torch.float32, "lse").shape != (B, h, L):
        raise RuntimeError("pbat_attn_fwd: S [B, h, L, b + 1] and lse [B, h, L]")
    call("gamer_pbat_attn_fwd", *args, float(scale), float(p_drop), int(seed), ptr(o1), ptr(o2), o1.stride(0), ptr(S), ptr(lse), ptr(ws),
         stream_ptr())


def pbat_n_partial(B, h):
    """Slabs of the attention backward's parameter gradients: n h workgroups, about one per CU (256)."""
    return max(1, min(B, 256 // max(1, h)))


def pbat_attn_bwd(proj, rel_m, rel_c, pos_m, pos_c, weights, types, keep, B, L, h, d, b, scale, p_drop, seed, S, lse, do1, do2, dproj,
                  drel_m, drel_c, w_partial, pos_partial):
    """gamer_pbat_attn_bwd: dproj = (dq1, dq2, dk1, dk2, dv1, dv2), drel_m / drel_c are written; w_partial [n, h, 4 (d d + d)] and
    pos_partial [n, h, 4, L, d] must be ZERO on entry (the caller sums them over n)."""
    args, ws = _pbat_common("pbat_attn_bwd", proj, rel_m, rel_c, pos_m, pos_c, weights, types, keep, B, L, h, d, b)
    H, NP = h * d, (b + 1) * (b + 1)
    for t in (do1, do2):
        _chk(t, torch.float32, "do")
        if t.shape != (B * L, H) or t.stride(1) != 1 or t.stride(0) != do1.stride(0):
            raise RuntimeError("pbat_attn_bwd: do1 / do2 [B L, h d] with one row stride")
    if len(dproj) != 6:
        raise RuntimeError("pbat_attn_bwd: six projection gradients")
    for t in dproj:
        _chk(t, torch.float32, "dproj")
        if t.shape != (B * L, H) or t.stride(1) != 1 or t.stride(0) != dproj[0].stride(0):
            raise RuntimeError("pbat_attn_bwd: the projection gradients must be [B L, h d] row-strided views with one row stride")
    n = w_partial.shape[0]
    if _dense(S, torch.float32, "S").shape != (B, h, L, b + 1) or _dense(lse, torch.float32, "lse").shape != (B, h, L) or \
            _dense(drel_m, torch.float32, "drel_m").shape != (B, NP, H) or _dense(drel_c, torch.float32, "drel_c").shape != (B, NP, H) or \
            _dense(w_partial, torch.float32, "w_partial").shape != (n, h, 4 * (d * d + d)) or \
            _dense(pos_partial, torch.float32, "pos_partial").shape != (n, h, 4, L, d) or not 0 < n <= B:
        raise RuntimeError("pbat_attn_bwd: S [B, h, L, b + 1], lse [B, h, L], drel [B, (b + 1)^2, h d], w_partial [n, h, 4 (d d + d)], "
                           "pos_partial [n, h, 4, L, d], 0 < n <= B")
    call("gamer_pbat_attn_bwd", *args, float(scale), float(p_drop), int(seed), ptr(S), ptr(lse), ptr(do1), ptr(do2),
         do1.stride(0), *[ptr(t) for t in dproj], dproj[0].stride(0), ptr(drel_m), ptr(drel_c), ptr(w_partial), ptr(pos_partial), n,
         ptr(ws), stream_ptr())


def _wass_pair(name, a, b, rows=None):
    R, H = a.shape if rows is None else (rows, a.shape[1])
    if _dense(a, torch.float32, name).dim() != 2 or _dense(b, torch.float32, name).shape != a.shape or a.shape[0] < R or R < 1:
        raise RuntimeError(f"{name}: two dense fp32 [rows, H] tensors of one shape")
    return R, H


def wass_rows_fwd(hm, hc, x, a):
    """x [R, 2 H] = -2 [hm, sqrt(clamp hc)], a [R] = |hm|^2 + sum hc (gamer_wass_rows_fwd)."""
    R, H = _wass_pair("wass_rows_fwd", hm, hc)
    if _dense(x, torch.float32, "x").shape != (R, 2 * H) or _dense(a, torch.float32, "a").shape != (R,):
        raise RuntimeError("wass_rows_fwd: x [R, 2 H], a [R]")
    call("gamer_wass_rows_fwd", ptr(hm), ptr(hc), R, H, ptr(x), ptr(a), stream_ptr())


def wass_rows_bwd(hm, hc, dx, da, dhm, dhc):
    R, H = _wass_pair("wass_rows_bwd", hm, hc)
    _wass_pair("wass_rows_bwd", dhm, dhc)
    if _dense(dx, torch.float32, "dx").shape != (R, 2 * H) or dhm.shape != hm.shape or \
            (da is not None and _dense(da, torch.float32, "da").shape != (R,)):
        raise RuntimeError("wass_rows_bwd: dx [R, 2 H], da [R] or None, dhm / dhc [R, H]")
    call("gamer_wass_rows_bwd", ptr(hm), ptr(hc), ptr(dx), ptr(da), R, H, ptr(dhm), ptr(dhc), stream_ptr())


def wass_table_fwd(Em, Ec, V, E2, c):
    """E2 [V, 2 H] = [Em, sqrt(clamp ec)], c [V] = |Em|^2 + sum ec, ec = ELU(Ec) + 1, over rows [0, V) (gamer_wass_table_fwd)."""
    V, H = _wass_pair("wass_table_fwd", Em, Ec, int(V))
    if _dense(E2, torch.float32, "E2").shape != (V, 2 * H) or _dense(c, torch.float32, "c").shape != (V,):
        raise RuntimeError("wass_table_fwd: E2 [V, 2 H], c [V]")
    call("gamer_wass_table_fwd", ptr(Em), ptr(Ec), V, H, ptr(E2), ptr(c), stream_ptr())


def wass_table_bwd(Em, Ec, V, dE2, dc, dEm, dEc):
    """rows [0, V) of dEm / dEc are written from dE2 [V, 2 H] and dc [V] (or None)."""
    V, H = _wass_pair("wass_table_bwd", Em, Ec, int(V))
    _wass_pair("wass_table_bwd", dEm, dEc, V)
    if _dense(dE2, torch.float32, "dE2").shape != (V, 2 * H) or dEm.shape[1] != H or \
            (dc is not None and _dense(dc, torch.float32, "dc").shape != (V,)):
        raise RuntimeError("wass_table_bwd: dE2 [V, 2 H], dc [V] or None, dEm / dEc [>= V, H]")
    call("gamer_wass_table_bwd", ptr(Em), ptr(Ec), ptr(dE2), ptr(dc), V, H, ptr(dEm), ptr(dEc), stream_ptr())


# ---- T5's attention (TIGER; csrc/t5_attention.hip, csrc/t5_attention_long.hip) --------------------------------------------------------
T5_MAX_S, T5_MAX_H, T5_HEAD_DIMS = 128, 16, (32, 64)


def t5_check_limits(Sq, Sk, h, d):
    """The limits of the T5 attention kernels, refused on the host before any launch."""
    if Sq < 1 or Sk < 1 or Sq > T5_MAX_S or Sk > T5_MAX_S or h < 1 or h > T5_MAX_H or d not in T5_HEAD_DIMS:
        raise NotImplementedError(f"T5 attention on the HIP path: Sq, Sk <= {T5_MAX_S}, heads <= {T5_MAX_H}, head size in "
                                  f"{T5_HEAD_DIMS} (got Sq={Sq}, Sk={Sk}, heads={h}, head size={d})")


def _t5_common(q, k, v, rel, keep, B, Sq, Sk, h, d, Bkv=None, check=None):
    (check or t5_check_limits)(Sq, Sk, h, d)
    Bkv = B if Bkv is None else Bkv
    for t, n, S, Bt in ((q, "q", Sq, B), (k, "k", Sk, Bkv), (v, "v", Sk, Bkv)):
        _chk(t, torch.float32, n)
        if t.dim() != 2 or t.shape != (Bt * S, h * d) or t.stride(1) != 1 or t.stride(0) % 4 or t.data_ptr() % 16:
            raise RuntimeError(f"t5 attention: {n} must be a [{B * S}, {h * d}] row-strided view (16-byte aligned, row stride % 4 == 0)")
    if rel is not None and _dense(rel, torch.float32, "rel").shape != (h, Sq + Sk - 1):
        raise RuntimeError(f"t5 attention: rel [{h}, {Sq + Sk - 1}]")
    if keep is not None and _dense(keep, torch.uint8, "keep").shape != (Bkv, Sk):
        raise RuntimeError(f"t5 attention: keep uint8 [{Bkv}, {Sk}]")


def t5_attn_fwd(q, k, v, rel, keep, B, Sq, Sk, h, d, causal, p_drop, seed, o, lse, kv_rows=None, kv_batch=None, _long=False):
    """gamer_t5_attn_fwd: q / o [B Sq, h d], k / v [B Sk, h d] (row-strided views), rel [h, Sq + Sk - 1] or None, keep uint8 [B, Sk] or
    None, lse [B, h, Sq].  No 1 / sqrt(d) scale.  kv_rows int32 [B] with kv_batch: k / v / keep hold kv_batch rows and row b reads
    row kv_rows[b] of them (values in [0, kv_batch): checked by the caller; decoding only - there is no backward for it)."""
    if (kv_rows is None) != (kv_batch is None) or (kv_rows is not None and _dense(kv_rows, torch.int32, "kv_rows").shape != (B,)):
        raise RuntimeError("t5_attn_fwd: kv_rows int32 [B] goes with kv_batch")
    _t5_common(q, k, v, rel, keep, B, Sq, Sk, h, d, kv_batch, t5_long_check_limits if _long else None)
    _chk(o, torch.float32, "o"), _dense(lse, torch.float32, "lse")
    if o.shape != (B * Sq, h * d) or o.stride(1) != 1 or lse.numel() != B * h * Sq:
        raise RuntimeError("t5_attn_fwd: o [B Sq, h d] and lse [B, h, Sq]")
    call("gamer_t5_attn_long_fwd" if _long else "gamer_t5_attn_fwd", ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v), v.stride(0), ptr(rel), ptr(keep), ptr(kv_rows), B, Sq, Sk,
         h, d, int(bool(causal)), float(p_drop), int(seed), ptr(o), o.stride(0), ptr(lse), stream_ptr())


def t5_n_slab(B, h):
    """Workgroup rows of the attention backward: n h workgroups, about two per CU (256 CUs), each walking the rows n apart."""
    return max(1, min(B, 512 // max(1, h)))


def t5_attn_bwd(q, k, v, rel, keep, B, Sq, Sk, h, d, causal, p_drop, seed, d_o, lse, dq, dk, dv, drel_partial, _long=False):
    """gamer_t5_attn_bwd: dq / dk / dv are written in full; drel_partial [n, h, Sq + Sk - 1] (None iff rel is None) is written in
    full by its n h workgroups (n <= B); without a bias n = t5_n_slab(B, h)."""
    _t5_common(q, k, v, rel, keep, B, Sq, Sk, h, d, check=t5_long_check_limits if _long else None)
    for t, n, S in ((d_o, "d_o", Sq), (dq, "dq", Sq), (dk, "dk", Sk), (dv, "dv", Sk)):
        _chk(t, torch.float32, n)
        if t.shape != (B * S, h * d) or t.stride(1) != 1:
            raise RuntimeError(f"t5_attn_bwd: {n} must be a [{B * S}, {h * d}] row-strided view")
    if _dense(lse, torch.float32, "lse").numel() != B * h * Sq:
        raise RuntimeError("t5_attn_bwd: lse [B, h, Sq]")
    if (rel is None) != (drel_partial is None):
        raise RuntimeError("t5_attn_bwd: drel_partial goes with the bias")
    n = t5_n_slab(B, h)
    if drel_partial is not None:
        n = drel_partial.shape[0]
        if _dense(drel_partial, torch.float32, "drel_partial").shape != (n, h, Sq + Sk - 1) or not 0 < n <= B:
            raise RuntimeError(f"t5_attn_bwd: drel_partial [n, {h}, {Sq + Sk - 1}], 0 < n <= B")
    args = (ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v), v.stride(0), ptr(rel), ptr(keep), B, Sq, Sk, h, d, int(bool(causal)),
            float(p_drop), int(seed), ptr(d_o), d_o.stride(0), ptr(lse), ptr(dq), dq.stride(0), ptr(dk), dk.stride(0), ptr(dv),
            dv.stride(0), ptr(drel_partial), n)
    if _long:
        row_ws = torch.empty(2, B, h, Sq, dtype=torch.float32, device=q.device)  # the softmax backward's row terms
        call("gamer_t5_attn_long_bwd", *args, ptr(row_ws), stream_ptr())
    else:
        call("gamer_t5_attn_bwd", *args, stream_ptr())


# the key-streaming family (csrc/t5_attention_long.hip): the same semantics for Sq, Sk <= 512, no buffer sized by the sequence
T5_LONG_MAX_S = 512


def t5_long_check_limits(Sq, Sk, h, d):
    """The limits of the key-streaming T5 attention kernels, refused on the host before any launch."""
    if Sq < 1 or Sk < 1 or Sq > T5_LONG_MAX_S or Sk > T5_LONG_MAX_S or h < 1 or h > T5_MAX_H or d not in T5_HEAD_DIMS:
        raise NotImplementedError(f"T5 attention on the HIP path (key-streaming kernels): Sq, Sk <= {T5_LONG_MAX_S}, heads <= {T5_MAX_H}, "
                                  f"head size in {T5_HEAD_DIMS} (got Sq={Sq}, Sk={Sk}, heads={h}, head size={d})")


def t5_attn_long_fwd(q, k, v, rel, keep, B, Sq, Sk, h, d, causal, p_drop, seed, o, lse, kv_rows=None, kv_batch=None):
    """gamer_t5_attn_long_fwd: the arguments of t5_attn_fwd, Sq, Sk <= 512."""
    t5_attn_fwd(q, k, v, rel, keep, B, Sq, Sk, h, d, causal, p_drop, seed, o, lse, kv_rows, kv_batch, _long=True)


def t5_attn_long_bwd(q, k, v, rel, keep, B, Sq, Sk, h, d, causal, p_drop, seed, d_o, lse, dq, dk, dv, drel_partial):
    """gamer_t5_attn_long_bwd: the arguments of t5_attn_bwd, Sq, Sk <= 512; allocates the row-term workspace [2, B, h, Sq]."""
    t5_attn_bwd(q, k, v, rel, keep, B, Sq, Sk, h, d, causal, p_drop, seed, d_o, lse, dq, dk, dv, drel_partial, _long=True)


def t5_bias_expand(table, bucket, rel):
    """rel [h, R] = table [num_buckets, h] at bucket int32 [R] (values in [0, num_buckets): checked by the caller)."""
    _dense(table, torch.float32, "table"), _dense(bucket, torch.int32, "bucket"), _dense(rel, torch.float32, "rel")
    nb, h = table.shape
    if rel.shape != (h, bucket.numel()) or bucket.dim() != 1:
        raise RuntimeError("t5_bias_expand: table [num_buckets, h], bucket [R], rel [h, R]")
    call("gamer_t5_bias_expand", ptr(table), ptr(bucket), nb, h, bucket.numel(), ptr(rel), stream_ptr())


def t5_bias_fold(drel_partial, bucket, dtable):
    """dtable [num_buckets, h] from drel_partial [layers, n, h, R]: slabs, offsets and layers summed in a fixed order."""
    _dense(drel_partial, torch.float32, "drel_partial"), _dense(bucket, torch.int32, "bucket"), _dense(dtable, torch.float32, "dtable")
    if drel_partial.dim() != 4 or bucket.shape != (drel_partial.shape[3],) or dtable.dim() != 2 or dtable.shape[1] != drel_partial.shape[2]:
        raise RuntimeError("t5_bias_fold: drel_partial [layers, n, h, R], bucket [R], dtable [num_buckets, h]")
    nl, n, h, R = drel_partial.shape
    call("gamer_t5_bias_fold", ptr(drel_partial), nl, n, h, R, ptr(bucket), dtable.shape[0], ptr(dtable), stream_ptr())


# ---- the packed (variable-length) forms of both families: rows one behind the other, no padding tokens ------------------------------
class T5Offsets:
    """The row offsets of a packed batch: ``host`` int32 [n + 1] on the CPU (what every argument check reads, so that no call copies
    from the device) and ``dev``, its device copy, which the kernels read.  ``total`` = host[n] rows, ``max_len`` the longest row.
    Refused here, before anything touches the library: offsets that do not start at 0 or decrease."""

    def __init__(self, host, device=None, dev=None):
        host = torch.as_tensor(host).detach()
        if host.is_cuda or host.dim() != 1 or host.numel() < 2 or host.dtype not in (torch.int32, torch.int64):
            raise ValueError("T5Offsets: a CPU int tensor of n + 1 >= 2 row offsets")
        if int(host[0]) != 0:
            raise ValueError(f"T5Offsets: offsets start at 0 (got {int(host[0])})")
        lens = host[1:] - host[:-1]
        if int(lens.min()) < 0:
            raise ValueError(f"T5Offsets: offsets decrease at row {int((lens < 0).nonzero()[0, 0])}")
        if int(host[-1]) >= 2 ** 31:
            raise ValueError("T5Offsets: more than 2^31 - 1 rows")
        self.host = host.to(torch.int32).contiguous()
        self.n, self.total, self.max_len = host.numel() - 1, int(host[-1]), int(lens.max())
        self.dev = dev if dev is not None else (self.host.to(device) if device is not None else None)

    @classmethod
    def from_lengths(cls, lengths, device=None):
        """the offsets of rows of ``lengths`` tokens (CPU int tensor [n], every entry >= 0)"""
        lengths = torch.as_tensor(lengths).detach().to("cpu", torch.int64).flatten()
        if lengths.numel() < 1 or int(lengths.min()) < 0:
            raise ValueError("T5Offsets.from_lengths: n >= 1 lengths, none negative")
        return cls(torch.cat([lengths.new_zeros(1), lengths.cumsum(0)]), device)

    @classmethod
    def uniform(cls, n, S, device=None):
        """dense rows of S tokens each (the decoder side of a cross attention)"""
        return cls(torch.arange(n + 1, dtype=torch.int64) * S, device)


def _t5_packed_common(name, q, k, v, rel, q_off, k_off, B, max_sq, max_sk, h, d, Bkv, _long):
    (t5_long_check_limits if _long else t5_check_limits)(max_sq, max_sk, h, d)
    for off, what, n, max_s in ((q_off, "q_start", B, max_sq), (k_off, "k_start", Bkv, max_sk)):
        if not isinstance(off, T5Offsets) or off.n != n:
            raise RuntimeError(f"{name}: {what} must be the T5Offsets of {n} rows")
        if off.max_len > max_s:
            lens = off.host[1:] - off.host[:-1]
            raise ValueError(f"{name}: row {int(lens.argmax())} of {what} holds {off.max_len} tokens, more than max {max_s}")
        if off.total < 1:
            raise ValueError(f"{name}: {what} holds no token")
        if off.dev is None or not off.dev.is_cuda or off.dev.dtype != torch.int32 or off.dev.numel() != n + 1 or not off.dev.is_contiguous():
            raise RuntimeError(f"{name}: {what} needs its int32 [{n + 1}] device copy")
    for t, n, T in ((q, "q", q_off.total), (k, "k", k_off.total), (v, "v", k_off.total)):
        _chk(t, torch.float32, n)
        if t.dim() != 2 or t.shape != (T, h * d) or t.stride(1) != 1 or t.stride(0) % 4 or t.data_ptr() % 16:
            raise RuntimeError(f"{name}: {n} must be a [{T}, {h * d}] row-strided view (16-byte aligned, row stride % 4 == 0)")
    if rel is not None and _dense(rel, torch.float32, "rel").shape != (h, max_sq + max_sk - 1):
        raise RuntimeError(f"{name}: rel [{h}, {max_sq + max_sk - 1}]")


def t5_attn_packed_fwd(q, k, v, rel, q_off, k_off, B, max_sq, max_sk, h, d, causal, p_drop, seed, o, lse, kv_rows=None, kv_batch=None,
                       _long=False):
    """gamer_t5_attn_packed_fwd: q / o [Tq, h d], k / v [Tk, h d] (row-strided views), q_off / k_off the rows' T5Offsets, rel
    [h, max_sq + max_sk - 1] or None, lse [h, Tq].  (max_sq, max_sk) is the shape of the dense run that the call replaces: bias
    offsets and dropout counters are those of that run.  kv_rows int32 [B] with kv_batch: k_off holds kv_batch rows."""
    name = "t5_attn_long_packed_fwd" if _long else "t5_attn_packed_fwd"
    if (kv_rows is None) != (kv_batch is None) or (kv_rows is not None and _dense(kv_rows, torch.int32, "kv_rows").shape != (B,)):
        raise RuntimeError(f"{name}: kv_rows int32 [B] goes with kv_batch")
    _t5_packed_common(name, q, k, v, rel, q_off, k_off, B, max_sq, max_sk, h, d, B if kv_batch is None else kv_batch, _long)
    _chk(o, torch.float32, "o"), _dense(lse, torch.float32, "lse")
    if o.shape != (q_off.total, h * d) or o.stride(1) != 1 or lse.numel() != h * q_off.total:
        raise RuntimeError(f"{name}: o [Tq, h d] and lse [h, Tq]")
    call("gamer_" + name, ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v), v.stride(0), ptr(rel), ptr(q_off.dev), ptr(k_off.dev),
         q_off.host.data_ptr(), k_off.host.data_ptr(), ptr(kv_rows), B, 0 if kv_batch is None else kv_batch, max_sq, max_sk, h, d,
         int(bool(causal)), float(p_drop), int(seed), ptr(o), o.stride(0), ptr(lse), stream_ptr())


def t5_attn_packed_bwd(q, k, v, rel, q_off, k_off, B, max_sq, max_sk, h, d, causal, p_drop, seed, d_o, lse, dq, dk, dv, drel_partial,
                       _long=False):
    """gamer_t5_attn_packed_bwd: dq / dk / dv (the layouts of q / k / v) are written in full; drel_partial
    [n, h, max_sq + max_sk - 1] as in t5_attn_bwd."""
    name = "t5_attn_long_packed_bwd" if _long else "t5_attn_packed_bwd"
    _t5_packed_common(name, q, k, v, rel, q_off, k_off, B, max_sq, max_sk, h, d, B, _long)
    for t, n, T in ((d_o, "d_o", q_off.total), (dq, "dq", q_off.total), (dk, "dk", k_off.total), (dv, "dv", k_off.total)):
        _chk(t, torch.float32, n)
        if t.shape != (T, h * d) or t.stride(1) != 1:
            raise RuntimeError(f"{name}: {n} must be a [{T}, {h * d}] row-strided view")
    if _dense(lse, torch.float32, "lse").numel() != h * q_off.total:
        raise RuntimeError(f"{name}: lse [h, Tq]")
    if (rel is None) != (drel_partial is None):
        raise RuntimeError(f"{name}: drel_partial goes with the bias")
    n = t5_n_slab(B, h)
    if drel_partial is not None:
        n = drel_partial.shape[0]
        if _dense(drel_partial, torch.float32, "drel_partial").shape != (n, h, max_sq + max_sk - 1) or not 0 < n <= B:
            raise RuntimeError(f"{name}: drel_partial [n, {h}, {max_sq + max_sk - 1}], 0 < n <= B")
    args = (ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v), v.stride(0), ptr(rel), ptr(q_off.dev), ptr(k_off.dev), q_off.host.data_ptr(),
            k_off.host.data_ptr(), B, max_sq, max_sk, h, d, int(bool(causal)), float(p_drop), int(seed), ptr(d_o), d_o.stride(0), ptr(lse),
            ptr(dq), dq.stride(0), ptr(dk), dk.stride(0), ptr(dv), dv.stride(0), ptr(drel_partial), n)
    if _long:
        row_ws = torch.empty(2, h, q_off.total, dtype=torch.float32, device=q.device)  # the softmax backward's row terms
        call("gamer_" + name, *args, ptr(row_ws), stream_ptr())
    else:
        call("gamer_" + name, *args, stream_ptr())


def t5_attn_long_packed_fwd(q, k, v, rel, q_off, k_off, B, max_sq, max_sk, h, d, causal, p_drop, seed, o, lse, kv_rows=None, kv_batch=None):
    """gamer_t5_attn_long_packed_fwd: the arguments of t5_attn_packed_fwd, max_sq, max_sk <= 512."""
    t5_attn_packed_fwd(q, k, v, rel, q_off, k_off, B, max_sq, max_sk, h, d, causal, p_drop, seed, o, lse, kv_rows, kv_batch, _long=True)


def t5_attn_long_packed_bwd(q, k, v, rel, q_off, k_off, B, max_sq, max_sk, h, d, causal, p_drop, seed, d_o, lse, dq, dk, dv, drel_partial):
    """gamer_t5_attn_long_packed_bwd: the arguments of t5_attn_packed_bwd, max_sq, max_sk <= 512; allocates the row terms [2, h, Tq]."""
    t5_attn_packed_bwd(q, k, v, rel, q_off, k_off, B, max_sq, max_sk, h, d, causal, p_drop, seed, d_o, lse, dq, dk, dv, drel_partial, _long=True)


def t5_attn_candidates(q, k, v, keep, B, R, Sk, h, d, o, k_off=None):
    """gamer_t5_attn_candidates: the decoder's cross attention for any number R of query rows per user.  q / o [B R, h d]
    (row-strided views; user b's rows are b R .. b R + R - 1), k / v [B Sk, h d] with keep uint8 [B, Sk] or None - or, with ``k_off``
    (the keys' T5Offsets of B rows), the packed [Tk, h d] rows, Sk their bound and no keep.  No bias, no causality, no dropout, no
    1 / sqrt(d), no lse.  The kernel's limits (Sk <= 128, h <= 16, d in (32, 64), alignment) are refused by the library, which names
    the entry point in gamer_last_error."""
    name = "t5_attn_candidates"
    if min(B, R, Sk, h, d) < 1:
        raise RuntimeError(f"{name}: B, R, Sk, h, d >= 1 (got {B}, {R}, {Sk}, {h}, {d})")
    if k_off is not None:
        if keep is not None:
            raise RuntimeError(f"{name}: packed keys take no keep")
        if not isinstance(k_off, T5Offsets) or k_off.n != B:
            raise RuntimeError(f"{name}: k_off must be the T5Offsets of {B} rows")
        if k_off.max_len > Sk:
            lens = k_off.host[1:] - k_off.host[:-1]
            raise ValueError(f"{name}: row {int(lens.argmax())} of k_start holds {k_off.max_len} tokens, more than max {Sk}")
        if k_off.total < 1:
            raise ValueError(f"{name}: k_start holds no token")
        if k_off.dev is None or not k_off.dev.is_cuda or k_off.dev.dtype != torch.int32 or k_off.dev.numel() != B + 1 or \
                not k_off.dev.is_contiguous():
            raise RuntimeError(f"{name}: k_start needs its int32 [{B + 1}] device copy")
    Tk = B * Sk if k_off is None else k_off.total
    for t, n, rows in ((q, "q", B * R), (k, "k", Tk), (v, "v", Tk), (o, "o", B * R)):
        _chk(t, torch.float32, n)
        if t.dim() != 2 or t.shape != (rows, h * d) or t.stride(1) != 1:
            raise RuntimeError(f"{name}: {n} must be a [{rows}, {h * d}] row-strided view")
    if keep is not None and _dense(keep, torch.uint8, "keep").shape != (B, Sk):
        raise RuntimeError(f"{name}: keep uint8 [{B}, {Sk}]")
    call("gamer_t5_attn_candidates", ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v), v.stride(0), ptr(keep),
         ptr(k_off.dev) if k_off is not None else None, k_off.host.data_ptr() if k_off is not None else None, B, R, Sk, h, d, ptr(o),
         o.stride(0), stream_ptr())
