"""Restatements for the PBATransformer tests: the two routers on the host (plain Python over the ids) and the whole model as
fp32 torch ops on any device.  Written from the model's description (position = place inside the item, behaviour = the item's
leading token through behavior_maps, the feed-forward layer on cat(x, behavior_embedding[b]) by the expert of the position); it
imports nothing from the reference.  The attention and the T5 frame are t5_attention_ref's."""
import torch

import t5_attention_ref as ref
import tiger_weights as tw


def route_host(ids, cfg, decoder: bool):
    """(position [B, S], behaviour [B, S], bad) as lists: the routers' rule on ids (a list of rows or a tensor); ``bad`` counts the
    positions whose behaviour is used and whose slot token behavior_maps does not hold (their behaviour is given as 0)"""
    rows = ids.tolist() if hasattr(ids, "tolist") else ids
    P, pad, eos = cfg["num_positions"], cfg["pad_token_id"], cfg["eos_token_id"]
    use_beh, moe = cfg["use_behavior_token"], cfg["Moe_behavior_only"]
    maps = {int(k): int(v) for k, v in cfg["behavior_maps"].items()}
    pos, beh, bad = [], [], 0
    for row in rows:
        S = len(row)
        p_row, b_row = [], []
        for s, tok in enumerate(row):
            special = tok in (pad, eos)
            if decoder:
                inside, r, slot = 1 <= s <= P, s - 1, 1
                used = inside and S > 1
            else:
                inside, r, slot = s < cfg["n_positions"] * P, s % P, s - s % P
                used = s < (S // P) * P
            p = 0
            if inside and not special:
                p = ((1 if r == 0 else 2) if use_beh else 1) if moe else r + 1
            b = 0
            if use_beh and used and r != 0 and not special:
                if row[slot] in maps:
                    b = maps[row[slot]] + 1
                else:
                    bad += 1
            p_row.append(p)
            b_row.append(b)
        pos.append(p_row)
        beh.append(b_row)
    return pos, beh, bad


def restated_model(sd, cfg, ids, am, labels, temperature, dev=ref.DEV, dtype=torch.float32):
    """PBATransformerForConditionalGeneration's forward as plain torch ops: (loss, logits, {name: grad})"""
    from gamer_amd.tiger import bucket_vector
    Pm = {k: v.to(dev).to(dtype).clone().requires_grad_(True) for k, v in sd.items() if k not in tw.TIED[1:]}
    h, d, eps, D = cfg["num_heads"], cfg["d_kv"], cfg["layer_norm_epsilon"], cfg["d_model"]
    n_exp = 2 if cfg["Moe_behavior_only"] else cfg["num_positions"] + 1
    E = Pm["shared.weight"]
    rms = lambda x, w: w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))
    heads = lambda x: x.view(x.shape[0], x.shape[1], h, d).permute(0, 2, 1, 3)

    def attn(pre, xq, xkv, rel, keep, causal):
        q, k, v = xq @ Pm[pre + "q.weight"].t(), xkv @ Pm[pre + "k.weight"].t(), xkv @ Pm[pre + "v.weight"].t()
        ctx, _ = ref.attention(heads(q), heads(k), heads(v), rel, keep, causal, None)
        return ctx.permute(0, 2, 1, 3).reshape(xq.shape[0], xq.shape[1], h * d) @ Pm[pre + "o.weight"].t()

    def ffn(f, x, pos, beh, sparse, inject):
        if inject:
            x = torch.cat([x, Pm[f + "mlp.behavior_embedding.weight"][beh]], -1)
        one = lambda name, rows: torch.relu(rows @ Pm[f + name + ".wi.weight"].t()) @ Pm[f + name + ".wo.weight"].t()
        if not sparse:
            return one("mlp.mlp", x)
        out = torch.zeros(*x.shape[:-1], D, device=x.device, dtype=x.dtype)
        for e in range(n_exp):
            sel = pos == e
            out = out + torch.where(sel[..., None], one(f"mlp.experts.expert_{e}", x), torch.zeros_like(out))
        return out

    def stack(name, tokens, n_layers, causal, keep, enc=None):
        x = E[tokens]
        S = x.shape[1]
        pos, beh, _ = route_host(tokens.cpu(), cfg, causal)
        pos, beh = torch.tensor(pos, device=x.device), torch.tensor(beh, device=x.device)
        sparse_layers = cfg["sparse_layers_decoder" if causal else "sparse_layers_encoder"]
        inject_layers = cfg["behavior_injection_decoder" if causal else "behavior_injection_encoder"]
        bucket = bucket_vector(S, not causal, cfg["relative_attention_num_buckets"], cfg["relative_attention_max_distance"]).long().to(x.device)
        rel = Pm[f"{name}.block.0.layer.0.SelfAttention.relative_attention_bias.weight"][bucket].t()
        for l in range(n_layers):
            b = f"{name}.block.{l}.layer."
            x = x + attn(b + "0.SelfAttention.", rms(x, Pm[b + "0.layer_norm.weight"]), rms(x, Pm[b + "0.layer_norm.weight"]), rel,
                         None if causal else keep, causal)
            if enc is not None:
                x = x + attn(b + "1.EncDecAttention.", rms(x, Pm[b + "1.layer_norm.weight"]), enc, None, keep, False)
            f = b + ("2." if enc is not None else "1.")
            x = x + ffn(f, rms(x, Pm[f + "layer_norm.weight"]), pos, beh, l in sparse_layers, l in inject_layers)
        return rms(x, Pm[f"{name}.final_layer_norm.weight"])
    keep = am.to(dev) != 0
    enc = stack("encoder", ids.to(dev), cfg["num_layers"], False, keep)
    dec_in = torch.zeros_like(labels)
    dec_in[:, 1:] = labels[:, :-1]
    dec_in[dec_in == -100] = 0
    out = stack("decoder", dec_in.to(dev), cfg["num_decoder_layers"], True, keep, enc) * D ** -0.5
    logits = out @ E.t()
    loss = torch.nn.functional.cross_entropy((logits / temperature).view(-1, logits.shape[-1]), labels.to(dev).view(-1), ignore_index=-100)
    loss.backward()
    return loss.detach(), logits.detach(), {k: v.grad for k, v in Pm.items()}
