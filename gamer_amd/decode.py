"""Evaluation path of the SMB decoder: trie-constrained beam search over the HIP engine.

Mirrors what ``test_SMB_decoder.py:test_single_behavior`` obtains from
``model.generate(..., max_new_tokens=4, num_beams=k, num_return_sequences=k, prefix_allowed_tokens_fn=...,
early_stopping=True)`` (ref:SeqRec/tasks/test_SMB_decoder.py:163-180) with the per-behaviour ``Trie`` of
``prefix_allowed_tokens_fn_by_last_token`` (ref:SeqRec/generation/trie.py:5-104; built at
test_SMB_decoder.py:470-500): the same sequences in the same order and the same ``sequences_scores``.

* The trie lives on the device as a CSR array; ``gamer_trie_logprobs`` does log-softmax + constraint + beam
  score per row and ``gamer_trie_advance`` moves the beams' trie nodes (csrc/decode.hip).  The reference walks a
  Python dict per (sample, beam) per step on the host.
* Beam bookkeeping follows transformers' ``GenerationMixin._beam_search`` for this call: top 2k of k*V
  candidates, the best k continue, the best k of the last step are the hypotheses, score = sum of log-probs /
  number of new tokens.  No EOS can be produced (the trie never allows it).
* K/V cache (``DecodeSession``): the prompt runs once per sample and its keys / values are stored once per sample
  (the reference stores num_beams copies); a generation step pushes one token per beam through the layers and
  ``gamer_attn_decode``.  ``use_cache=False`` re-runs the whole sequence each step instead; both give the same
  beams.  The two things the reference's cache freezes are explicit (``act_zero_col``, ``uniform_len``;
  Engine.forward).  One reference defect is NOT reproduced: its cross-attention cache lives on the module and is not re-ordered with the beams
  (model.py:569,785,844-860), which perturbs samples whose target row is "empty" (oracle/decode_oracle.py,
  tests/test_decode.py quantify it).
* ``Engine(dtype="bf16")`` (Qwen3Multi): the search runs in the arithmetic of the ``--bf16`` run - bf16 prompt and generated (self)
  caches, ``gamer_attn_decode_bf16`` (csrc/decode_bf16.hip), the bf16 twins on the shadow weights, fp32 residual stream and
  logits.  A row without an allowed key gives 0 in bf16, so none of the three things the fp32 path does for the uniform-average
  quirk exists there (``uniform_len``, ``uniform``, the generated cross rows and their slot order): cached and re-run path are
  one computation, ``reorder_cross_cache`` changes nothing (tests/test_decode_bf16_gpu.py).
* ``score_items`` (end of the file): the exact log-likelihood of GIVEN items on the same cached path - rows are (user, candidate)
  pairs, any number per user, through ``gamer_attn_candidates`` (csrc/candidates.hip); fp32 engines.
"""
from __future__ import annotations

import os
from typing import Dict, List, Sequence, Tuple

import torch

from . import ops


class ItemTrie:
    """CSR trie over item token sequences (node 0 = root).  ``get(prefix)`` is the host-side ``Trie.get``."""

    def __init__(self, sequences: Sequence[Sequence[int]], device="cuda", pad_token_id: int = 4):
        """``pad_token_id``: the tokenizer's pad id (config.pad_token_id; 4 in the shipped config.json), which
        test_SMB_decoder.py:473-474 adds to the item-ending tokens."""
        nodes: List[Dict[int, int]] = [{}]
        for seq in sequences:
            cur = 0
            for t in seq:
                t = int(t)
                nxt = nodes[cur].get(t)
                if nxt is None:
                    nxt = len(nodes)
                    nodes[cur][t] = nxt
                    nodes.append({})
                cur = nxt
        start, tok, child = [0], [], []
        for d in nodes:
            for t, c in d.items():             # insertion order, as the reference's dict
                tok.append(t)
                child.append(c)
            start.append(len(tok))
        self.nodes = nodes
        self.n_items = len(sequences)
        # tokens that end an item, plus the pad id (test_SMB_decoder.py:473-474)
        self.last_tokens = {int(seq[-1]) for seq in sequences} | {int(pad_token_id)}
        i32 = dict(dtype=torch.int32, device=device)
        self.child_start = torch.tensor(start, **i32)
        self.child_tok = torch.tensor(tok if tok else [0], **i32)
        self.child_node = torch.tensor(child if child else [0], **i32)

    def get(self, prefix: Sequence[int]) -> List[int]:
        cur = 0
        for t in prefix:
            cur = self.nodes[cur].get(int(t))
            if cur is None:
                return []
        return list(self.nodes[cur].keys())


def prefix_allowed_tokens(trie: ItemTrie):
    """Callable with the signature of the reference's ``prefix_allowed_tokens_fn_by_last_token`` result
    (trie.py:90-104) for host-side use; ``Qwen3MultiWithTemperature.generate`` takes the trie it carries."""
    last_tokens = {seq_last for seq_last in trie.last_tokens}

    def fn(batch_id: int, sentence) -> List[int]:
        s = [int(t) for t in sentence]
        i = len(s) - 1
        while i >= 0 and s[i] not in last_tokens:
            i -= 1
        return trie.get(s[i + 1:])
    fn.trie = trie
    return fn


def trie_from_callable(fn, input_ids, max_new_tokens: int, device="cuda", pad_token_id: int = 4) -> ItemTrie:
    """Device trie equivalent to an arbitrary ``prefix_allowed_tokens_fn(batch_id, sentence) -> allowed token ids`` for
    prompts that end with a target behaviour token - the closure the evaluation task builds per behaviour
    (ref:SeqRec/tasks/test_SMB_decoder.py:470-500, ref:SeqRec/generation/trie.py:90-104) passed to ``generate`` unchanged.
    The callable is walked depth first from one prompt per distinct final token (its answers only depend on the tokens
    since the last item-ending token, i.e. on [behaviour token] + generated), ``max_new_tokens`` levels deep: one host
    call per trie node, once - the result is cached on the callable (``fn._gamer_tries``).
    LIMITS (checked where they can be): the callable must not depend on ``batch_id`` or on prompt tokens before the last one -
    the first level is cross-checked on a second row with the same final token when the batch has one, and a callable that
    allows nothing after the prompt raises; a callable with other semantics than trie.py:90-104 needs its own ItemTrie."""
    ids = input_ids.detach().cpu()
    cache = getattr(fn, "_gamer_tries", None)
    if cache is None:
        cache = {}
        try:
            fn._gamer_tries = cache
        except AttributeError:                      # a callable without a __dict__: walk it every time
            pass
    last = ids[:, -1]
    key = (tuple(sorted(set(int(t) for t in last.tolist()))), int(max_new_tokens), str(device))
    if key in cache:
        return cache[key]
    sequences = []
    for tok in key[0]:
        b = int((last == tok).nonzero()[0])
        prompt = ids[b].tolist()

        def walk(prefix):
            if len(prefix) == max_new_tokens:
                sequences.append([tok] + prefix)
                return
            allowed = [int(t) for t in fn(b, torch.tensor(prompt + prefix))]
            if not allowed and prefix:                          # an item shorter than max_new_tokens
                sequences.append([tok] + prefix)
            for t in allowed:
                walk(prefix + [t])
        first = sorted(int(t) for t in fn(b, torch.tensor(prompt)))
        if not first:
            raise ValueError(f"prefix_allowed_tokens_fn allows no token after a prompt ending in {tok}: prompts must end with the "
                             "target behaviour token (ref:SeqRec/tasks/test_SMB_decoder.py:470-500)")
        others = (last == tok).nonzero().flatten().tolist()
        if len(others) > 1:                                     # the same final token in another row must give the same first level
            b2 = int(others[-1])
            if sorted(int(t) for t in fn(b2, ids[b2])) != first:
                raise ValueError("prefix_allowed_tokens_fn depends on more than the tokens since the last item-ending token "
                                 f"(rows {b} and {b2} end in {tok} and get different continuations): build an ItemTrie per row group")
        walk([])
    trie = ItemTrie(sequences, device=device, pad_token_id=pad_token_id)
    cache[key] = trie
    return trie


class _DecodeStatic:
    """Buffers of the cached decode path at FIXED addresses, kept on the engine per (batch, prompt length, beams, new tokens, ...):
    an evaluation run decodes many batches of one shape and reuses them; with GAMER_DECODE_GRAPH=1 the per-token step - ~350
    launches - is captured into one hipGraph per step index once two sessions of the shape have run eagerly (kernel attributes
    set, weight maxima registered) and replayed from then on, bit-identical to the eager step (tests/test_decode.py).
    MEASURED on MI355X / ROCm 7.2 (tools/decode_leg.py): the replay is no faster than the eager step - 2.45 against 2.40 ms per token
    at 16 users x 20 beams, 2.28 / 2.28 at 64, 4.08 / 3.98 at 256: a kernel node costs the ~7 us of dispatch an eager launch costs,
    and at 256 users the step is GPU time anyway (tools/decode_step_kernels.py: gamer_attn_decode 1.73 of 3.6 ms) - so the graph
    is OFF by default; what would shorten the step is FEWER launches, not cheaper ones.
    The buffers belong to the latest session of the shape: ``claims`` counts the sessions that have taken them."""

    def __init__(self):
        self.kp: Dict[Tuple[int, str], torch.Tensor] = {}
        self.vp: Dict[Tuple[int, str], torch.Tensor] = {}
        self.qkvp: Dict[Tuple[int, str], torch.Tensor] = {}     # fp32 engines: the layers' own q|k|v buffers (vp = their v columns)
        self.gen = None
        self.buf = None
        self.small: Dict[str, torch.Tensor] = {}
        self.graphs: Dict[int, "torch.cuda.CUDAGraph"] = {}
        self.sessions = 0            # sessions of this shape that have run so far
        self.sig = None              # state of the engine's maxima cache the graphs were captured against
        self.claims = 0              # sessions that have taken these buffers (the latest one owns them)


def _graphs_enabled() -> bool:
    return os.environ.get("GAMER_DECODE_GRAPH", "0") == "1"


def _check_generation_dtype(engine):
    """Generation on a bf16 engine is built for the default variant (Qwen3Multi) only."""
    if engine.dtype != "f32" and engine.variant != "multi":
        raise NotImplementedError(f"generation on a dtype={engine.dtype!r} engine is built for the default variant (Qwen3Multi), "
                                  f"not for variant {engine.variant!r}: generate from an fp32 engine of it")


def _session_kw(engine, session_ids, extended_session_ids) -> dict:
    """The session ids of a session engine ("session", "qwen3_session", "qwen3_session_moe") on the device - required there -
    and {} for the others."""
    if engine.variant not in ("session", "qwen3_session", "qwen3_session_moe"):
        return {}
    if session_ids is None or extended_session_ids is None:
        raise ValueError("a session engine needs session_ids and extended_session_ids")
    return dict(session_ids=session_ids.to(engine.device, torch.int64),
                extended_session_ids=extended_session_ids.to(engine.device, torch.int64))


class DecodeSession:
    """K/V cache of one generation run + the single-token forward over it (model.py:118-121, 784-785).

    The prompt is run once per SAMPLE (HF expands it to num_beams copies first) and its keys / values are kept
    once per sample; only the generated positions are per beam.  ``step`` pushes one token per beam through the
    layers with the ordinary row kernels (norms, GEMMs with M = B*num_beams rows, SwiGLU) - all new tokens of a
    step sit at the same position, hence in the same position-routed expert - and ``gamer_attn_decode``.
    GAMER_DECODE_GRAPH=1: from the third session of a shape on the step is a hipGraph replay (``_DecodeStatic``: measured neutral).
    This class is Qwen3Multi's (and Qwen3SessionMulti's) session and the core every model shares; a model's own parts are the
    hooks ``_eval_forward`` (its prompt pass), ``_row_inputs`` (the step's per-row inputs) and ``_layer_tail`` (a layer after
    its self-attention block) - ``Qwen3DecodeSession`` overrides them for the plain Qwen3 baselines.
    ONE LIVE SESSION PER SHAPE: the sessions of an engine with the same (batch, prompt length, beams, new tokens, model, cross
    cache order, matmul form, dtype) share their buffers (``_DecodeStatic``).  Creating a session takes them over; ``step`` and
    ``reorder`` of an older session of that shape then raise RuntimeError instead of attending over the newer one's caches
    (``beam_search`` runs one session at a time)."""

    _STATIC_SLOT = "_decode_static"      # the engine attribute that holds this kind of session's buffers, by shape
    _REORDERS = True                     # rows are beams: the generated caches follow ``reorder`` at the start of a step

    def __init__(self, engine, input_ids, attention_mask, actions, num_beams: int, max_new_tokens: int,
                 session_ids=None, extended_session_ids=None, reorder_cross_cache: bool = False):
        """``reorder_cross_cache=False`` (default) is the reference as shipped: its cross-attention K/V cache lives on
        the module (model.py:569, 785, 844-860) and HF's beam search only re-orders ``past_key_values``, so the
        generated positions' cross K/V rows stay in the beam SLOT that wrote them.  They are masked for every query
        except target rows with no lower-level key in the prompt, whose uniform average then reads V rows of other
        beams.  ``True`` re-orders the cross cache with the beams like the self cache (the consistent variant; the
        only one the cache-free re-run path can reproduce).
        ``session_ids`` / ``extended_session_ids`` [B, L0] (the test collator's layout, collator.py:176-195) for a
        "session" engine: the prompt runs with the session masks; the generated tokens then see every kept key in
        the self attention and the prompt's last cross-mask row in the cross attention, exactly as for Qwen3Multi
        (Qwen3SessionMulti/model.py:598-613, 716-728), with RoPE positions last extended id + 1, + 2, ...
        (:969-982)."""
        _check_generation_dtype(engine)
        cfg, dev = engine.cfg, engine.device
        self.eng, self.nb, self.tmax = engine, num_beams, max_new_tokens
        # bf16 engine (Qwen3Multi): bf16 caches and step activations on the shadow weights, fp32 residual stream and logits.  A row
        # without an allowed key gives 0 there (csrc/attention_bf16.hip), so the generated positions' cross K / V - masked for every
        # other row - are never read: no cross rows are cached and ``reorder_cross_cache`` changes nothing
        self.bf16 = engine.dtype == "bf16"
        self.reorder_cross_cache = bool(reorder_cross_cache) and not self.bf16
        self.B, self.L0 = input_ids.shape
        B, L0 = self.B, self.L0
        self.N = N = B * num_beams
        sess = _session_kw(engine, session_ids, extended_session_ids)
        statics = engine.__dict__.setdefault(self._STATIC_SLOT, {})
        key = (B, L0, num_beams, max_new_tokens, engine.variant, self.reorder_cross_cache, engine.matmul, engine.dtype)
        st = statics.get(key)
        if st is None:
            if len(statics) >= 4:                     # (a few shapes at most: the buffers of a shape are ~2.5 GB at 256 users)
                statics.pop(next(iter(statics)))
            st = statics[key] = _DecodeStatic()
        self.st = st
        st.claims += 1                                # (before the prompt pass overwrites the caches of an older session)
        self.claim = st.claims
        ids0 = input_ids.to(dev, torch.int64)
        am0 = attention_mask.to(dev, torch.int64)
        act0 = None if actions is None else actions.to(dev, torch.int64)
        nq, nkv, dh = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
        self.NQ, self.NKV = nq * dh, nkv * dh
        QKV = self.NQ + 2 * self.NKV
        T0 = B * L0
        f32 = dict(dtype=torch.float32, device=dev)
        self.kp, self.vp = st.kp, st.vp

        # fp32 engines: the prompt pass writes every layer's q|k|v projection and rotated keys straight into the session's buffers
        # (Engine.forward(kv_dest=...): the V cache is the v columns of the layer's own q|k|v buffer, row stride QKV) - no copy of 2 x
        # 98 MB per layer and kind - and the maxima the three-piece decode attention needs are the ones the prompt pass's own
        # attention used (the producers left them in the engine's maxima cache): no gamer_absmax_f32 pass over the caches either
        direct = engine.dtype == "f32" and os.environ.get("GAMER_DECODE_DIRECT_KV", "1") != "0"      # (0: the copying path, A/B and tests)
        want_amax = (engine._amax is not None and engine.matmul == "split3" and os.environ.get("GAMER_DECODE_ATTN_SPLIT", "1") != "0")
        prompt_amax = {}

        def dest(layer, kind):
            kk = (layer, kind)
            if kk not in st.qkvp or st.qkvp[kk].shape[0] != T0:
                st.qkvp[kk] = torch.empty(T0, QKV, **f32)
                st.kp[kk] = torch.empty(T0, self.NKV, **f32)
                st.vp[kk] = st.qkvp[kk][:, self.NQ + self.NKV:]
            return st.qkvp[kk], st.kp[kk]

        def sink(layer, kind, k, v):
            kk = (layer, kind)
            if direct:
                if want_amax:       # (called in front of the layer's attention: the slots the producers of k / v left for it, if they did)
                    sk = engine._amax.peek(k, (1, 0, T0, self.NKV, k.stride(0)))
                    sv = engine._amax.peek(v, (1, 0, T0, self.NKV, v.stride(0)))
                    if sk and sv:
                        prompt_amax[kk] = (sk, sv)
                return
            if kk not in st.kp:
                st.kp[kk] = k.clone()
                st.vp[kk] = v.contiguous().clone()       # v is a column slice of the qkv buffer
            else:
                st.kp[kk].copy_(k)
                st.vp[kk].copy_(v)
        self._eval_forward(engine, ids0, am0, act0, sess, L0, kv_sink=sink, kv_dest=dest if direct else None, last_row_logits=True)
        if sess:
            engine.check_inputs()
        # last-row logits of every sample: the head ran on B rows, not on the whole prompt
        self.prefill_logits = engine.last_logits_buf

        def keep(name, value):
            """the step's small inputs at fixed addresses (the captured step reads them)"""
            value = value.contiguous()
            t = st.small.get(name)
            if t is None or t.shape != value.shape or t.dtype != value.dtype:
                st.small[name] = t = value.clone()
            else:
                t.copy_(value)
            return t
        self.ok_self = keep("ok_self", am0.to(torch.int32))
        # RoPE position of the token generated at step t, per beam row: pos_last + t - for a session model the prompt's largest
        # extended id + t; None: position L0 + t - 1 for every row
        self.pos_last = None
        if sess:
            self.pos_last = keep("pos_last", sess["extended_session_ids"].max(dim=1).values.to(torch.int32).repeat_interleave(num_beams))
        self._row_inputs(keep, ids0, am0, act0, sess)
        if st.gen is None:
            # the activations between the fp32 residual stream x and the fp32 logits have the engine's activation dtype; a bf16
            # session keeps generated rows for the self blocks only
            act = dict(dtype=engine.act_dtype, device=dev)
            st.gen = {kk: (torch.zeros(N, max_new_tokens, self.NKV, **act), torch.zeros(N, max_new_tokens, self.NKV, **act))
                      for kk in self.kp if not (self.bf16 and kk[1] == "cross")}
            H, I = cfg.hidden_size, cfg.intermediate_size
            st.buf = dict(x=[torch.empty(N, H, **f32) for _ in range(2)], h=torch.empty(N, H, **act),
                          qkv=torch.empty(N, QKV, **act), q=torch.empty(N, self.NQ, **act), k=torch.empty(N, self.NKV, **act),
                          ao=torch.empty(N, self.NQ, **act), gu=torch.empty(N, 2 * I, **act), hm=torch.empty(N, I, **act),
                          xn=torch.empty(N, H, **act), logits=torch.empty(N, engine.ws.ldl, **f32),
                          gen_tmp=torch.empty(N, max(1, max_new_tokens - 1), self.NKV, **act))
            if self.bf16:         # the head's bf16 logits (padding columns stay zero), widened into ``logits`` for the beam scores
                st.buf["logits16"] = torch.zeros(N, engine.ws.ldl, **act)
            if cfg.cross_attention_decoder or cfg.behavior_injection_decoder:
                # Qwen3Multi's layers: the state after the cross block, its o_proj and gate outputs, and the FFN input widened
                # by the injected behaviour embedding (without these layers the FFN reads h)
                st.buf["x"].append(torch.empty(N, H, **f32))
                st.buf.update(op=torch.empty(N, H, **act), gate=torch.empty(N, H, **act),
                              hin=torch.empty(N, H + cfg.behavior_embedding_dim, **act))
            st.small["tok"] = torch.zeros(N, dtype=torch.int64, device=dev)
            st.small["parent"] = torch.arange(N, dtype=torch.int64, device=dev)
        # (stale generated rows of an earlier session are never read: gamer_attn_decode takes the number of valid positions)
        self.gen, self.buf = st.gen, st.buf
        self._pending_reorder = False
        self.t = 0
        # matmul = "split3": the decode attention in the three-piece fp16 form too - the maxima of the prompt K / V caches, which do not
        # change during the generation, measured once (GAMER_DECODE_ATTN_SPLIT=0: the fp32-MFMA kernel)
        self.kv_amax = {}
        if want_amax:
            if len(prompt_amax) == len(self.kp):
                self.kv_amax = prompt_amax
            else:
                with ops.f32_matmul("split3"), engine._amax:
                    for kk in self.kp:
                        kpt, vpt = self.kp[kk], self.vp[kk]
                        self.kv_amax[kk] = (ops.absmax_slot(kpt, 1, 0, kpt.shape[0], kpt.shape[1], kpt.stride(0)),
                                            ops.absmax_slot(vpt, 1, 0, vpt.shape[0], vpt.shape[1], vpt.stride(0)))
        # the maxima cache as this session found it after the prompt pass: what a captured step was recorded against
        am_ = engine._amax
        self._sig = None if am_ is None else (len(am_._wkeys), am_.used, 0 if am_.planes is None else am_.planes.data_ptr())
        if st.graphs and st.sig != self._sig:
            st.graphs.clear()                       # (another weight set / slot layout: record again)
            st.sessions = 0
        st.sessions += 1

    @staticmethod
    def _eval_forward(engine, ids, am, act, sess: dict, L0: int, **kw):
        """The model's evaluation forward of prompts of length ``L0`` (+ generated tokens): a session's prompt pass and the
        cache-free re-run of ``beam_search``.  Qwen3Multi: with the two things the reference's cache freezes, ``act_zero_col``
        and ``uniform_len`` (Engine.forward)."""
        engine.forward(ids, am, act, train=False, act_zero_col=L0 - 1, uniform_len=L0, **sess, **kw)

    def _row_inputs(self, keep, ids0, am0, act0, sess: dict):
        """The step's per-row inputs besides ``ok_self`` and a session model's ``pos_last``.  Qwen3Multi: the cross mask of the
        new rows = kept keys of a lower level than the target behaviour (the cached last mask row, model.py:603-617; no allowed
        key -> uniform over every key), and the router outputs of the generated tokens (router.py:158-195 in decode mode):
        behaviour index + 1 of the target item's behaviour token, for the FFN injection and the cross-attention biases."""
        ok_cross = (am0 != 0) & (act0 < act0[:, -1:])
        if sess:
            sid0 = sess["session_ids"]
            ok_cross &= sid0 < sid0[:, -1:]              # Qwen3SessionMulti/model.py:582-584, last prompt row
        ok_cross[:, -1] = False
        self.ok_cross = keep("ok_cross", ok_cross.to(torch.int32))
        self.uniform_cross = keep("uniform_cross", (~ok_cross.any(1)).to(torch.int32))
        self.beh = keep("beh", (self.eng.lut[ids0[:, -1]].to(torch.int32) + 1).repeat_interleave(self.nb))

    def _own(self):
        if self.st.claims != self.claim:
            raise RuntimeError("a newer DecodeSession of the same shape has taken this engine's decode buffers: only the latest "
                               "session of a shape can step (one live session per shape)")

    def reorder(self, parent: torch.Tensor):
        """Beams were re-ordered: the generated part of the SELF cache follows its beam (the prompt part is shared);
        the cross cache only with ``reorder_cross_cache`` (see __init__).  The rows move at the start of the next step
        (in place, the positions generated so far only), so that the move is part of the captured step."""
        self._own()
        self.st.small["parent"].copy_(parent)
        self._pending_reorder = True

    @ops.scoped_f32_matmul(lambda self, *a: self.eng.matmul)
    @ops.scoped_amax(lambda self, *a: self.eng._amax)
    def step(self, tokens: torch.Tensor) -> torch.Tensor:
        """tokens [N] int64: the token just appended to every beam.  Returns the next-token logits [N, ld].
        (matmul="split3": runs inside the engine's maxima cache - the parameters keep the slots of the prompt pass, which
        measured them once (they cannot change during a generation), the producers of the step's activations hand their
        maxima to the GEMMs (gamer_amax_sink) - instead of two gamer_absmax_f32 launches per GEMM and token.)"""
        self._own()
        st = self.st
        st.small["tok"].copy_(tokens)
        self.t += 1
        t = self.t
        reorder = self._pending_reorder
        self._pending_reorder = False
        if t >= 2 and not reorder:
            st.small["parent"].copy_(torch.arange(self.N, dtype=torch.int64, device=tokens.device))
        g = st.graphs.get(t)
        if g is not None:
            g.replay()
            return self.buf["logits"]
        if _graphs_enabled() and not self.bf16 and st.sessions >= 3 and tokens.is_cuda:      # (a bf16 session always steps eagerly)
            self.eng.rope(self.L0 + self.tmax)          # (cached tables: nothing may be built on the host during the capture)
            if self.eng._amax is not None:
                self.eng._amax.reserve(512)             # (a fresh slot pool is zero-filled at allocation: not inside the graph)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._step_body(t)
            st.graphs[t] = g
            st.sig = self._sig
            g.replay()
            return self.buf["logits"]
        self._step_body(t)
        return self.buf["logits"]

    def _step_body(self, t: int):
        eng, cfg, b = self.eng, self.eng.cfg, self.buf
        N, L0, NQ, NKV = self.N, self.L0, self.NQ, self.NKV
        H, eps = cfg.hidden_size, float(cfg.rms_norm_eps)
        if t >= 2 and self._REORDERS:
            # the beams were re-ordered after the last step: the t - 1 generated positions follow them
            parent = self.st.small["parent"]
            for key, (kg, vg) in self.gen.items():
                if key[1] == "cross" and not self.reorder_cross_cache:
                    continue
                tmp = b["gen_tmp"].view(-1)[:N * (t - 1) * NKV].view(N, t - 1, NKV)
                torch.index_select(kg[:, :t - 1], 0, parent, out=tmp)
                kg[:, :t - 1] = tmp
                torch.index_select(vg[:, :t - 1], 0, parent, out=tmp)
                vg[:, :t - 1] = tmp
        cos, sin = eng.rope(L0 + self.tmax)
        if self.pos_last is None:                        # the table row of the new tokens' common position
            p = L0 + t - 1
            self._rope = (cos[p:p + 1], sin[p:p + 1], None)
        else:                                            # per beam row; the table is indexed through pos_ids
            self._rope = (cos, sin, (self.pos_last + t).contiguous())
        # the per-head RMSNorm + RoPE as the q|k|v projection's epilogue: at these row counts the projection runs on the 128 x 128 kernel
        # either way (the activation-stationary kernel starts at 16 k rows), so the epilogue only removes a launch and a pass per
        # attention and token (in the train step, where it would displace the faster kernel, it measured 9 ms slower)
        self._fuse_qk = (eng.dtype == "f32" and os.environ.get("GAMER_DECODE_FUSE_QK", "1") != "0"
                         and ops.qkv_fused_ok(b["h"], N, NQ + 2 * NKV))
        x, x1 = b["x"][:2]
        ops.embedding_fwd(self.st.small["tok"], eng.params["model.embed_tokens.weight"], x)
        # x holds the layer input and receives the layer output; x1 is the state after the self-attention block
        # (W: norm weights and tables, always the fp32 masters; eng.Wm: what the GEMMs read - the masters, or a bf16 engine's shadow copies)
        for l in range(cfg.num_hidden_layers):
            W = eng.W[l]
            ops.rmsnorm_fwd(x, W.ln1, eps, b["h"])
            self._attend(t, "self", l, W.self_attn)
            ops.gemm(b["ao"], NQ, 1, eng.Wm[l].self_attn["o"], NQ, 1, x1, H, N, H, NQ, resid=x)
            self._layer_tail(t, l, W, x, x1)
        ops.rmsnorm_fwd(x, eng.params["model.norm.weight"], eps, b["xn"])
        if self.bf16:
            # bf16 logits against the bf16 copy of the tied table, as the scoring forward's head gives them; fp32 for gamer_trie_logprobs
            lg16 = b["logits16"]
            ops.linear_fwd(b["xn"], H, eng.shadow.params16["model.embed_tokens.weight"], H, lg16, lg16.stride(0), N, cfg.vocab_size, H)
            b["logits"].copy_(lg16)
            return
        ops.linear_fwd(b["xn"], H, eng.params["model.embed_tokens.weight"], H, b["logits"], b["logits"].stride(0), N,
                       cfg.vocab_size, H)

    def _attend(self, t: int, kind: str, layer: int, Wa: dict, act_idx=None):
        """Attention of the new rows (input b["h"]) into b["ao"]: q|k|v with the per-head RMSNorm + RoPE, the new position
        appended to the layer's generated K / V, ``gamer_attn_decode`` over the prompt's and the generated keys.  ``act_idx``:
        the behaviour biases of a cross block."""
        cfg, b = self.eng.cfg, self.buf
        N, H, NQ, NKV = self.N, cfg.hidden_size, self.NQ, self.NKV
        nq, nkv, QKV = cfg.num_attention_heads, cfg.num_key_value_heads, NQ + 2 * NKV
        eps, scale = float(cfg.rms_norm_eps), float(cfg.head_dim) ** -0.5
        cos, sin, pos_ids = self._rope
        is_self = kind == "self"
        bias = {} if is_self else dict(bias_q=Wa["bq"], bias_k=Wa["bk"], bias_v=Wa["bv"], act_idx=act_idx)
        if self.bf16:
            # the bf16 twins on the shadow weights; only a self block appends its new position, and a cross block - whose generated keys
            # no row can read - attends the prompt cache alone (gamer_attn_decode_bf16 with gen_ok = 0 never touches kg / vg)
            Wm = self.eng.Wm[layer]
            ops.linear_fwd(b["h"], H, (Wm.self_attn if is_self else Wm.cross_attn)["qkv"], H, b["qkv"], QKV, N, QKV, H)
            ops.qknorm_rope_fwd(b["qkv"], 1, nq, nkv, Wa["qn"], Wa["kn"], eps, cos, sin, b["q"], b["k"], pos_ids=pos_ids, **bias)
            kg, vg = self.gen[(layer, "self")]
            if is_self:
                ops.kv_append_bf16(b["k"], b["qkv"][:, NQ + NKV:], kg, vg, t - 1)
            ops.attn_decode_bf16(b["q"], self.kp[(layer, kind)], self.vp[(layer, kind)], self.ok_self if is_self else self.ok_cross,
                                 kg, vg, t, is_self, self.B, self.nb, self.L0, nq, nkv, scale, b["ao"])
            return
        if self._fuse_qk:
            ops.gemm(b["h"], H, 1, Wa["qkv"], H, 1, b["qkv"], QKV, N, QKV, H,
                     qknorm=dict(wq=Wa["qn"], wk=Wa["kn"], eps=eps, cos=cos, sin=sin, q_rot=b["q"], k_rot=b["k"], pos_ids=pos_ids,
                                 S=1, nq=nq, nkv=nkv, **bias))
        else:
            ops.linear_fwd(b["h"], H, Wa["qkv"], H, b["qkv"], QKV, N, QKV, H)
            ops.qknorm_rope_fwd(b["qkv"], 1, nq, nkv, Wa["qn"], Wa["kn"], eps, cos, sin, b["q"], b["k"], pos_ids=pos_ids, **bias)
        kg, vg = self.gen[(layer, kind)]
        ops.kv_append(b["k"], b["qkv"][:, NQ + NKV:], kg, vg, t - 1)
        self._attn_rows(layer, kind, kg, vg, t, scale)

    def _attn_rows(self, layer: int, kind: str, kg, vg, t: int, scale: float):
        """The fp32 step attention of the new rows b["q"] over the layer's prompt cache and their own generated positions, into
        b["ao"]: ``gamer_attn_decode`` (num_beams * G <= 64 rows per sample; the three-piece form with the prompt caches' maxima)."""
        cfg, b, is_self = self.eng.cfg, self.buf, kind == "self"
        ops.attn_decode(b["q"], self.kp[(layer, kind)], self.vp[(layer, kind)], self.ok_self if is_self else self.ok_cross,
                        kg, vg, t, is_self, None if is_self else self.uniform_cross, self.B, self.nb, self.L0,
                        cfg.num_attention_heads, cfg.num_key_value_heads, scale, b["ao"], amax=self.kv_amax.get((layer, kind)))

    def _layer_tail(self, t: int, l: int, W, x, x1):
        """Layer ``l`` after its self-attention block (output x1): the layer output into x.  Qwen3Multi: the cross block with
        the behaviour biases and the output gate, the behaviour injection and the position-routed expert FFN."""
        eng, cfg, b, N = self.eng, self.eng.cfg, self.buf, self.N
        H, I, E, NQ, eps = cfg.hidden_size, cfg.intermediate_size, cfg.num_ffn_experts, self.NQ, float(cfg.rms_norm_eps)
        Wm = eng.Wm[l]                                   # the GEMMs' operands (W itself in fp32)
        xc = x1
        if W.cross:
            xc = b["x"][2]
            ops.rmsnorm_fwd(x1, W.ln2, eps, b["h"])
            self._attend(t, "cross", l, W.cross_attn, self.beh)
            ops.linear_fwd(b["ao"], NQ, Wm.cross_attn["o"], NQ, b["op"], H, N, H, NQ)
            ops.linear_fwd(b["h"], H, Wm.cross_attn["gate"], H, b["gate"], H, N, H, H)
            ops.silu_gate_fwd(b["op"], b["gate"], xc, resid=x1)
        # the expert of the new tokens' common position (router.py:28-54 table, the same for every row); a dense layer's one MLP
        pos = (self.L0 + t - 1) % cfg.num_positions
        if not (W.sparse and W.gated and not cfg.Moe_behavior_only):
            # the FFN ablation forms (dense layer, PBATransformer experts, behaviour-only routing: semantic tokens have no expert)
            eng.ffn_rows(W, pos, xc, self.beh if W.inject else None, x, Wm)
            return
        hin, din = b.get("hin", b["h"]), W.din
        ops.rmsnorm_fwd(xc, W.ln3, eps, hin, din)
        if W.inject:
            ops.rowtable_fwd(W.beh, self.beh, hin, din, H)
        e = pos + 1                                      # position-routed expert (router.py:83-104), same for every row
        if eng._amax is not None and eng.matmul == "split3":
            # the whole stacked weight with every row in expert e's group: the tensor the prompt pass measured and cut (its maximum
            # slot and packed pieces are reused; a row slice is another tensor to the maxima cache - two gamer_absmax_f32 launches
            # and two cuts of the weight per layer and token)
            key = f"expert_offsets_{e}"
            if key not in self.st.small:           # rows [0, N) belong to expert e, every other group is empty
                self.st.small[key] = torch.tensor([0] * (e + 1) + [N] * (E - e), dtype=torch.int32, device=eng.device)
            grp = dict(groups=E, group_offsets=self.st.small[key])
            ops.linear_fwd(hin, din, W.gu, din, b["gu"], 2 * I, N, 2 * I, din, strideB=2 * I * din, **grp)
            ops.swiglu_fwd_ld(b["gu"], 2 * I, N, I, 0.0, 0, b["hm"])
            ops.gemm(b["hm"], I, 1, W.down, I, 1, x, H, N, H, I, strideB=H * I, resid=xc, **grp)
            return
        ops.linear_fwd(hin, din, Wm.gu[e * 2 * I:(e + 1) * 2 * I], din, b["gu"], 2 * I, N, 2 * I, din)      # gate | up of expert e
        ops.swiglu_fwd_ld(b["gu"], 2 * I, N, I, 0.0, 0, b["hm"])
        ops.gemm(b["hm"], I, 1, Wm.down[e * H:(e + 1) * H], I, 1, x, H, N, H, I, resid=xc)


class Qwen3DecodeSession(DecodeSession):
    """K/V cache + single-token step of the plain Qwen3 baselines (``Engine(variant="qwen3")`` / ``"qwen3_session"``): self
    attention and a dense MLP per layer.  The prompt pass runs with transformers' generate() positions ``cumsum(attention_mask) - 1``
    (gamer_causal_prep builds them on the device) and writes every layer's q|k|v and rotated keys in place; the token
    generated at step t is rotated by (number of kept prompt tokens) + t - 1, per row - a left-padded prompt by its own offset.
    Qwen3Session (``session_ids`` / ``extended_session_ids`` [B, L0], required): the prompt pass runs with the session mask
    and the extended ids as positions (gamer_session_prep); the generated tokens see every kept key and are rotated by
    max(extended_session_ids[row]) + t, with no padding offset (Qwen3Session/model.py:293-309)."""

    def __init__(self, engine, input_ids, attention_mask, num_beams: int, max_new_tokens: int, session_ids=None,
                 extended_session_ids=None):
        _check_generation_dtype(engine)
        super().__init__(engine, input_ids, attention_mask, None, num_beams, max_new_tokens, session_ids, extended_session_ids)

    @staticmethod
    def _eval_forward(engine, ids, am, act, sess: dict, L0: int, **kw):
        """RoPE positions from the extended session ids (Qwen3Session) or, as transformers' generate(), from the attention mask."""
        engine.forward(ids, am, train=False, **(sess or dict(rope_from_mask=True)), **kw)

    def _row_inputs(self, keep, ids0, am0, act0, sess: dict):
        """The plain baseline's pos_last: the number of kept prompt tokens - 1 (gamer_causal_prep's next_pos - 1), per row."""
        if not sess:
            self.pos_last = keep("pos_last", (self.eng.ws.mask["next_pos"] - 1).repeat_interleave(self.nb))

    def _layer_tail(self, t: int, l: int, W, x, x1):
        """The dense SwiGLU MLP."""
        cfg, b, N = self.eng.cfg, self.buf, self.N
        H, I = cfg.hidden_size, cfg.intermediate_size
        ops.rmsnorm_fwd(x1, W.ln2, float(cfg.rms_norm_eps), b["h"])
        ops.linear_fwd(b["h"], H, W.gu, H, b["gu"], 2 * I, N, 2 * I, H)
        ops.swiglu_fwd_ld(b["gu"], 2 * I, N, I, 0.0, 0, b["hm"])
        ops.gemm(b["hm"], I, 1, W.down, I, 1, x, H, N, H, I, resid=x1)


def _check_moe_generation(engine, L0: int, max_new_tokens: int):
    """What a Qwen3Moe generation is built for: prompts ending with the target behaviour token (the trie starts there and the
    generated tokens take its behaviour), and columns inside the router's table (the reference indexes past it)."""
    if not engine.cfg.use_behavior_token:
        raise NotImplementedError("generation needs behaviour tokens (the prompt ends with the target behaviour token); "
                                  "a model trained with use_behavior_token=False is trained and scored, not generated from")
    if L0 + max_new_tokens - 1 > engine.max_len():
        raise ValueError(f"prompt of {L0} tokens + {max_new_tokens} new ones exceeds the router's table, n_positions * "
                         f"num_positions + 1 = {engine.max_len()} (router.py:46-60)")


class Qwen3MoeDecodeSession(DecodeSession):
    """K/V cache + single-token step of Qwen3Moe (``Engine(variant="qwen3moe")``): Qwen3Multi's layers without a cross block,
    so no cross caches.  The prompt pass runs with the causal + key-padding mask and generate()'s positions
    ``cumsum(attention_mask) - 1`` (gamer_moe_router_prep builds both); the token generated at step t is rotated by (number
    of kept prompt tokens) + t - 1 per row, routed to the expert of its column L0 + t - 1 (the reference router's
    ``cache_position`` rule) and, with behaviour tokens, injected with the behaviour of the prompt's last token (the target
    item's behaviour token)."""

    def __init__(self, engine, input_ids, attention_mask, num_beams: int, max_new_tokens: int):
        _check_generation_dtype(engine)
        _check_moe_generation(engine, input_ids.shape[1], max_new_tokens)
        super().__init__(engine, input_ids, attention_mask, None, num_beams, max_new_tokens)

    @staticmethod
    def _eval_forward(engine, ids, am, act, sess: dict, L0: int, **kw):
        engine.forward(ids, am, train=False, rope_from_mask=True, **kw)

    def _row_inputs(self, keep, ids0, am0, act0, sess: dict):
        eng = self.eng
        self.pos_last = keep("pos_last", (eng.next_pos - 1).repeat_interleave(self.nb))
        if eng.cfg.use_behavior_token:
            beh = (eng.lut[ids0[:, -1]].to(torch.int32) + 1).clamp_(min=0)
        else:
            beh = torch.zeros(self.B, dtype=torch.int32, device=eng.device)
        self.beh = keep("beh", beh.repeat_interleave(self.nb))


class Qwen3SessionMoeDecodeSession(Qwen3MoeDecodeSession):
    """K/V cache + single-token step of Qwen3SessionMoe (``Engine(variant="qwen3_session_moe")``): ``Qwen3MoeDecodeSession``
    with a session model's prompt pass and positions.  The prompt pass runs with the session mask as key spans, the extended
    ids as positions and the router by column (gamer_session_moe_prep, ``session_ids`` / ``extended_session_ids`` [B, L0]
    required); the generated tokens see every kept key (model.py:444-455), are rotated by max(extended_session_ids[row]) + t
    (``DecodeSession``'s ``pos_last`` of a session model; model.py:688-703) and routed to the expert of their column."""

    def __init__(self, engine, input_ids, attention_mask, num_beams: int, max_new_tokens: int, session_ids=None,
                 extended_session_ids=None):
        _check_generation_dtype(engine)
        _check_moe_generation(engine, input_ids.shape[1], max_new_tokens)
        DecodeSession.__init__(self, engine, input_ids, attention_mask, None, num_beams, max_new_tokens, session_ids,
                               extended_session_ids)

    @staticmethod
    def _eval_forward(engine, ids, am, act, sess: dict, L0: int, **kw):
        engine.forward(ids, am, train=False, **sess, **kw)

    def _row_inputs(self, keep, ids0, am0, act0, sess: dict):
        """The behaviour of the prompt's last token for the injection layers (``pos_last`` is the session model's)."""
        beh = (self.eng.lut[ids0[:, -1]].to(torch.int32) + 1).clamp_(min=0)
        self.beh = keep("beh", beh.repeat_interleave(self.nb))


def _check_moe_action_generation(engine, L0: int, max_new_tokens: int):
    """What a Qwen3MoeAction generation is built for besides ``_check_moe_generation``: a prompt of n P + 1 tokens (whole items
    and the target behaviour token) and new tokens inside the target item, so that every generated token has the target
    behaviour's action and the only column the reference's cache freezes at action 0 is the prompt's last."""
    _check_moe_generation(engine, L0, max_new_tokens)
    P = int(engine.cfg.num_positions)
    if L0 % P != 1 % P or max_new_tokens > P:
        raise ValueError(f"a Qwen3MoeAction generation takes prompts of n * num_positions + 1 tokens and at most num_positions "
                         f"new ones (got {L0} and {max_new_tokens}, num_positions = {P})")


class Qwen3MoeActionDecodeSession(Qwen3MoeDecodeSession):
    """K/V cache + single-token step of Qwen3MoeAction (``Engine(variant="qwen3moe_action")``): ``Qwen3MoeDecodeSession`` whose
    rows sit in up to ``num_behavior`` experts per step.  The prompt pass is gamer_moe_action_router_prep's: the last column of
    the n P + 1 prompt tokens keeps the reference's action 0 (the action table's eos slot) in the cache.  The token generated
    at step t runs in expert (num_experts - 1) * (a_row - 1) + table[(L0 + t - 1) % P], a_row = the behaviour of the row's
    last prompt token, which is also its injected behaviour.  A row's behaviour never changes and beams stay inside their
    user, so the rows' expert lists (gamer_expert_lists over the [B, beams] index) are built once per session, one set per
    position of an item, at fixed addresses; a step sorts its rows through them for the grouped GEMMs as the forward pass
    does - no host loop over experts, no synchronisation."""

    def __init__(self, engine, input_ids, attention_mask, num_beams: int, max_new_tokens: int):
        _check_generation_dtype(engine)
        _check_moe_action_generation(engine, input_ids.shape[1], max_new_tokens)
        super().__init__(engine, input_ids, attention_mask, num_beams, max_new_tokens)

    @staticmethod
    def _eval_forward(engine, ids, am, act, sess: dict, L0: int, **kw):
        """The prompt pass, and the cache-free re-run with what the cache freezes: action 0 in column L0 - 1."""
        engine.forward(ids, am, train=False, rope_from_mask=True, act_zero_col=L0 - 1, **kw)

    def _row_inputs(self, keep, ids0, am0, act0, sess: dict):
        super()._row_inputs(keep, ids0, am0, act0, sess)
        eng, cfg = self.eng, self.eng.cfg
        P = int(cfg.num_positions)
        table = torch.tensor(cfg.position_experts(), dtype=torch.int32, device=eng.device)
        self.lists = {}
        for t in range(1, self.tmax):
            p = (self.L0 + t - 1) % P
            e = ((cfg.num_experts - 1) * (self.beh - 1) + table[p]).clamp_(min=0).to(torch.int32).view(self.B, self.nb)
            self.lists[p] = tuple(keep(f"action_{name}_{p}", v) for name, v in zip(("perm", "slot", "offsets"), eng.row_lists(e)))

    def _layer_tail(self, t: int, l: int, W, x, x1):
        """The FFN: a dense layer's one MLP, or the experts of the rows' (behaviour, position) pairs."""
        eng, b = self.eng, self.buf
        pos = (self.L0 + t - 1) % eng.cfg.num_positions
        beh = self.beh if W.inject else None
        if not W.sparse:
            eng.ffn_rows(W, pos, x1, beh, x, eng.Wm[l])
            return
        eng.ffn_rows_grouped(W, self.lists[pos], x1, beh, x, bufs=dict(hin=b.get("hin", b["h"]), gu=b["gu"], hm=b["hm"]))


@torch.no_grad()
def beam_search(engine, input_ids: torch.Tensor, attention_mask: torch.Tensor, actions: torch.Tensor, trie: ItemTrie,
                num_beams: int, max_new_tokens: int = 4, use_cache: bool = True, session_ids=None,
                extended_session_ids=None, reorder_cross_cache: bool = False, return_trace: bool = False):
    """input_ids / attention_mask / actions: [B, L0] left-padded prompts ending with the target behaviour token
    (``actions`` None for the "qwen3" baseline, which has no behaviour levels).
    Returns (sequences [B*num_beams, L0+max_new_tokens] int64, sequences_scores [B*num_beams] fp32), the beams of
    sample b at rows b*num_beams .., best first - the layout of HF's GenerateBeamOutput.
    ``use_cache=False`` re-runs the whole sequence every step (the cross-check of the cache path; it has no slots, so
    it needs ``reorder_cross_cache=True``).  ``reorder_cross_cache``: see ``DecodeSession`` (False = the reference).
    ``session_ids`` / ``extended_session_ids`` [B, L0]: required by a "session" engine (see DecodeSession).
    ``return_trace=True``: a third value, the list over the steps of (parent [B, nb] int64 - the beam slot each kept candidate
    continues -, token [B, nb] int64, running_score [B, nb] fp32 - the sum of its log-probs), best first.
    A ``dtype="bf16"`` engine (Qwen3Multi only) searches in the arithmetic it was trained in: a row without an allowed key gives
    0 there, so ``reorder_cross_cache`` is accepted and changes nothing, and the cached and the re-run path compute the same."""
    _check_generation_dtype(engine)
    bf16 = engine.dtype == "bf16"
    reorder_cross_cache = reorder_cross_cache or bf16          # (one and the same search in bf16: the re-run path may always run)
    trace = []
    qwen3 = engine.variant in ("qwen3", "qwen3_session")
    session_moe = engine.variant == "qwen3_session_moe"
    action_moe = engine.variant == "qwen3moe_action"
    moe = engine.variant == "qwen3moe" or session_moe or action_moe     # (no behaviour levels either: no actions, no cross cache)
    if not use_cache and not reorder_cross_cache and not (qwen3 or moe):
        raise ValueError("use_cache=False re-computes every position for its own beam: it can only reproduce "
                         "reorder_cross_cache=True (the shipped reference's un-reordered cross cache needs the cache)")
    cls = (Qwen3DecodeSession if qwen3 else Qwen3SessionMoeDecodeSession if session_moe else
           Qwen3MoeActionDecodeSession if action_moe else Qwen3MoeDecodeSession if moe else DecodeSession)
    if action_moe:
        _check_moe_action_generation(engine, input_ids.shape[1], max_new_tokens)
    elif moe:
        _check_moe_generation(engine, input_ids.shape[1], max_new_tokens)
    dev = engine.device
    B, L0 = input_ids.shape
    V = engine.cfg.vocab_size
    nb, K = num_beams, 2 * num_beams
    N = B * nb
    ids0 = input_ids.to(dev, torch.int64)
    am0 = attention_mask.to(dev, torch.int64)
    act0 = actions.to(dev, torch.int64) if not (qwen3 or moe) else None
    sess0 = _session_kw(engine, session_ids, extended_session_ids)
    seqs = ids0[:, None, :].expand(B, nb, L0).contiguous()
    run_scores = torch.zeros(B, nb, device=dev)
    run_scores[:, 1:] = -1e9                       # only beam 0 is live at the first step (HF)
    # trie node of every beam: the prefix since the last complete item is the target behaviour token
    node = torch.zeros(N, dtype=torch.int32, device=dev)
    nxt = torch.empty_like(node)
    ops.trie_advance(node, ids0[:, -1].repeat_interleave(nb).contiguous(), trie.child_start, trie.child_tok,
                     trie.child_node, nxt)
    node, nxt = nxt, node
    scores = torch.empty(N, V, device=dev)
    final = None
    if not use_cache:
        session = None
    elif qwen3:
        session = Qwen3DecodeSession(engine, ids0, am0, nb, max_new_tokens, **sess0)
    elif session_moe:
        session = Qwen3SessionMoeDecodeSession(engine, ids0, am0, nb, max_new_tokens, **sess0)
    elif action_moe:
        session = Qwen3MoeActionDecodeSession(engine, ids0, am0, nb, max_new_tokens)
    elif moe:
        session = Qwen3MoeDecodeSession(engine, ids0, am0, nb, max_new_tokens)
    else:
        session = DecodeSession(engine, ids0, am0, act0, nb, max_new_tokens, reorder_cross_cache=reorder_cross_cache, **sess0)
    last_tok = None
    for step in range(max_new_tokens):
        cur = L0 + step
        if session is not None:
            if step == 0:
                logits2d = session.prefill_logits
                rows = torch.arange(N, device=dev, dtype=torch.int32) // nb
            else:
                logits2d = session.step(last_tok)
                rows = torch.arange(N, device=dev, dtype=torch.int32)
        else:
            # the cache-free cross-check: the whole sequence again (the first step runs every sample's prompt once, HF runs
            # num_beams copies).  The generated tokens belong to the target item: the behaviour level and session id of its
            # behaviour token and the next extended ids, which makes the training masks equal to the cached ones
            flat, am, act, sess = ids0, am0, act0, sess0
            if step:
                flat = seqs.reshape(N, cur)
                am = torch.cat([am0, am0.new_ones(B, step)], 1).repeat_interleave(nb, 0)
                if act0 is not None:
                    act = torch.cat([act0, act0[:, -1:].expand(B, step)], 1).repeat_interleave(nb, 0)
                if sess0:
                    sid0, ext0 = sess0["session_ids"], sess0["extended_session_ids"]
                    ext = torch.cat([ext0, ext0[:, -1:] + torch.arange(1, step + 1, device=dev)[None, :]], 1)
                    sess = dict(session_ids=torch.cat([sid0, sid0[:, -1:].expand(B, step)], 1).repeat_interleave(nb, 0),
                                extended_session_ids=ext.repeat_interleave(nb, 0))
            cls._eval_forward(engine, flat, am, act, sess, L0)
            if sess:
                engine.check_inputs()
            logits2d = engine.ws.logits
            rows = (torch.arange(N, device=dev, dtype=torch.int32) // (nb if step == 0 else 1)) * cur + (cur - 1)
            if bf16:            # the last rows of the head's bf16 logits, widened for gamer_trie_logprobs
                logits2d = logits2d.index_select(0, rows.to(torch.int64)).to(torch.float32)
                rows = torch.arange(N, device=dev, dtype=torch.int32)
        ops.trie_logprobs(logits2d, rows, run_scores.reshape(N).contiguous(), node, trie.child_start, trie.child_tok,
                          V, scores)
        top_s, top_i = torch.topk(scores.view(B, nb * V), K)
        beam_i, tok = top_i // V, top_i % V
        cand = torch.cat([torch.gather(seqs, 1, beam_i[:, :, None].expand(B, K, cur)), tok[:, :, None]], 2)
        if return_trace:
            trace.append((beam_i[:, :nb].clone(), tok[:, :nb].clone(), top_s[:, :nb].clone()))
        if step == max_new_tokens - 1:
            final = (cand[:, :nb].reshape(N, cur + 1), (top_s[:, :nb] / max_new_tokens).reshape(N))
            break
        seqs = cand[:, :nb].contiguous()
        run_scores = top_s[:, :nb].contiguous()
        parent = (beam_i[:, :nb] + torch.arange(B, device=dev)[:, None] * nb).reshape(N)
        last_tok = tok[:, :nb].reshape(N).contiguous()
        if session is not None:
            session.reorder(parent)
        ops.trie_advance(node[parent].contiguous(), tok[:, :nb].reshape(N).contiguous(), trie.child_start,
                         trie.child_tok, trie.child_node, nxt)
        node, nxt = nxt.clone(), nxt
    return final + (trace,) if return_trace else final


# ---- exact scoring of given items on the cached decode path ---------------------------------------------------------------
class _ScoreRows:
    """Mixed in front of a decode session class: its rows are (user, candidate) pairs instead of beams.  Any number of rows per
    user - the step attention is ``gamer_attn_candidates`` (csrc/candidates.hip; fp32 MFMA in every fp32 matmul form, the GEMMs
    follow the engine's form) -, no beam re-ordering, and buffers of its own on the engine (``_score_static``), so that the
    beam-search sessions' buffers (``_decode_static``) are neither taken over nor evicted."""

    _STATIC_SLOT = "_score_static"
    _REORDERS = False

    def _attn_rows(self, layer: int, kind: str, kg, vg, t: int, scale: float):
        cfg, b, is_self = self.eng.cfg, self.buf, kind == "self"
        ops.attn_candidates(b["q"], self.kp[(layer, kind)], self.vp[(layer, kind)], self.ok_self if is_self else self.ok_cross,
                            kg, vg, t, is_self, None if is_self else self.uniform_cross, self.B, self.nb, self.L0,
                            cfg.num_attention_heads, cfg.num_key_value_heads, scale, b["ao"])

    @ops.scoped_f32_matmul(lambda self, *a: self.eng.matmul)
    @ops.scoped_amax(lambda self, *a: self.eng._amax)
    def score_step(self, tokens: torch.Tensor, t: int) -> torch.Tensor:
        """tokens [N] int64: token t - 1 of every row's item.  Returns the logits [N, ld] of the rows' token t.  ``t`` starts again
        at 1 for every chunk of candidates: the generated caches are overwritten from position 0 (positions >= t are never read)."""
        self._own()
        self.st.small["tok"].copy_(tokens)
        self.t = t
        self._step_body(t)
        return self.buf["logits"]


_SCORE_CLASSES: Dict[type, type] = {}


def _session_class(engine):
    """The decode session class of the engine's variant, whether its constructor takes ``actions`` and whether it takes the
    session ids."""
    v = engine.variant
    if v in ("qwen3", "qwen3_session"):
        return Qwen3DecodeSession, False, True
    if v == "qwen3_session_moe":
        return Qwen3SessionMoeDecodeSession, False, True
    if v == "qwen3moe_action":
        return Qwen3MoeActionDecodeSession, False, False
    if v == "qwen3moe":
        return Qwen3MoeDecodeSession, False, False
    if v in ("multi", "session"):
        return DecodeSession, True, True
    raise NotImplementedError(f"score_items: variant {v!r} has no decode session")


@torch.no_grad()
def score_items(engine, input_ids: torch.Tensor, attention_mask: torch.Tensor, actions: torch.Tensor, items: torch.Tensor,
                session_ids=None, extended_session_ids=None, max_rows: int = 65536) -> torch.Tensor:
    """Log-likelihood of GIVEN items after every user's prompt, on the cached decode path.

    input_ids / attention_mask / actions: [B, L0] left-padded prompts ending with the target behaviour token, as for ``beam_search``
    (``actions`` None for the models without behaviour levels; session engines need ``session_ids`` / ``extended_session_ids``).
    ``items``: [C, T] int64 - one list for every user - or [B, C, T], a list per user.
    Returns scores [B, C] fp32: scores[b, c] = (1 / T) * sum_t log_softmax(logits_t)[items[.., c, t]] over the whole vocabulary -
    what ``beam_search`` returns as ``sequences_scores`` for the same tokens in the cache-consistent semantics
    (``reorder_cross_cache=True``: every generated position's cross K/V belongs to its own row), i.e. what the cache-free re-run
    ``_eval_forward(prompt + item)`` computes.
    The prompt pass runs ONCE for the batch; token 0 is scored from the prefill logits (shared by a user's candidates); the
    candidates then go through T - 1 single-token steps in chunks of at most ``max_rows // B`` per user (rows = (user, candidate),
    ``gamer_attn_candidates`` as the step attention, ``gamer_token_logprob`` for a row's log-prob: no [N, V] log-softmax, no
    top-k, no re-ordering).  Generated caches and step buffers are sized by the chunk.  fp32 engines only.  Candidates that share
    a prefix are not merged: with 256-way codes nearly every depth-2 prefix of a catalogue belongs to one item."""
    if engine.dtype != "f32":
        raise NotImplementedError(f"score_items is built for fp32 engines, not for dtype={engine.dtype!r}: score from an fp32 "
                                  "engine of the model")
    cls, takes_actions, takes_sessions = _session_class(engine)
    if items.dim() not in (2, 3) or items.dtype != torch.int64:
        raise ValueError(f"score_items: items must be int64 [C, T] or [B, C, T], got {items.dtype} {tuple(items.shape)}")
    B, L0 = input_ids.shape
    if items.dim() == 3 and items.shape[0] != B:
        raise ValueError(f"score_items: items [B, C, T] has {items.shape[0]} lists for {B} users")
    C, T = items.shape[-2:]
    if C < 1 or T < 1:
        raise ValueError(f"score_items: empty item list {tuple(items.shape)}")
    if max_rows < B:
        raise ValueError(f"score_items: max_rows = {max_rows} < {B} users (one candidate per user is the smallest chunk)")
    if cls is Qwen3MoeActionDecodeSession:
        _check_moe_action_generation(engine, L0, T)
    elif issubclass(cls, Qwen3MoeDecodeSession):
        _check_moe_generation(engine, L0, T)
    dev, V = engine.device, engine.cfg.vocab_size
    n_chunks = -(-C // max(1, max_rows // B))
    chunk = -(-C // n_chunks)                                  # (balanced: the last chunk is padded by < n_chunks candidates)
    scls = _SCORE_CLASSES.get(cls)
    if scls is None:
        scls = _SCORE_CLASSES[cls] = type("Score" + cls.__name__, (_ScoreRows, cls), {})
    sess = dict(session_ids=session_ids, extended_session_ids=extended_session_ids) if takes_sessions else {}
    if takes_actions:
        session = scls(engine, input_ids, attention_mask, actions, chunk, T, reorder_cross_cache=True, **sess)
    else:
        session = scls(engine, input_ids, attention_mask, chunk, T, **sess)
    statics = engine.__dict__[scls._STATIC_SLOT]               # one shape of scoring buffers at a time (they are sized by the chunk)
    for k in [k for k, st in statics.items() if st is not session.st]:
        del statics[k]
    it = items.to(dev)
    if it.dim() == 2:
        it = it[None].expand(B, C, T)
    N = B * chunk
    user = (torch.arange(N, device=dev, dtype=torch.int32) // chunk).contiguous()
    out = torch.empty(B, n_chunks * chunk, dtype=torch.float32, device=dev)
    acc = torch.empty(N, dtype=torch.float32, device=dev)
    for ci in range(n_chunks):
        c0 = ci * chunk
        cols = torch.arange(c0, c0 + chunk, device=dev).clamp_(max=C - 1)      # (the last chunk repeats the last candidate)
        tok = it.index_select(1, cols).reshape(N, T).t().contiguous()           # [T, N]
        ops.token_logprob(session.prefill_logits, user, tok[0], V, acc)
        for t in range(1, T):
            logits = session.score_step(tok[t - 1], t)
            ops.token_logprob(logits, None, tok[t], V, acc, accumulate=True)
        out[:, c0:c0 + chunk] = acc.view(B, chunk)
    return out[:, :C] / T
