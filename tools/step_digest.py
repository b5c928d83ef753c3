"""GPU: loss and a digest of the flat gradient after one training step (forward + backward, dropout on) at B x 505 tokens, of the
ordered list of C entry points the step calls, of an evaluation forward with last_row_logits=True and of a short beam search -
two builds (of the library, or of the host code over one library) that claim the same bits and launches print the same line:
GAMER_LIB_PATH=<variant.so> python tools/step_digest.py [B] [f32|bf16] [matmul] [multi|session|qwen3|qwen3_session]
(the session models train and decode on sessions of mean 4 items)"""
import hashlib, os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gamer_amd
from gamer_amd import decode, ops, synthetic
from gamer_amd.config import Qwen3Config, Qwen3SessionConfig, synthetic_config
from gamer_amd.engine import Engine

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
dt = sys.argv[2] if len(sys.argv) > 2 else "f32"
mm = sys.argv[3] if len(sys.argv) > 3 else "split3"
model = sys.argv[4] if len(sys.argv) > 4 else "multi"
calls = []


def recording(fn):
    def wrapper(name, *args):
        calls.append(name)
        return fn(name, *args)
    return wrapper


for mod in (ops, getattr(gamer_amd, "modeling", None)):
    if mod is not None and hasattr(mod, "call"):
        mod.call = recording(mod.call)


def h(*ts):
    d = hashlib.sha256()
    for t in ts:
        d.update(t.detach().cpu().contiguous().numpy().tobytes())
    return d.hexdigest()[:16]


V = synthetic.vocab_size(256, 3)
if model == "qwen3":
    cfg = Qwen3Config(vocab_size=V, pad_token_id=synthetic.PAD_ID)
elif model == "qwen3_session":
    cfg = Qwen3SessionConfig(vocab_size=V, pad_token_id=synthetic.PAD_ID, num_positions=5, model_max_length=1024)
else:
    cfg = synthetic_config()
eng = Engine(cfg, temperature=0.7, variant=model, dtype=dt, matmul=mm)
eng.init_weights(seed=0)
sessions = model in ("session", "qwen3_session")
sm = 4.0 if sessions else None
batch = {k: v.cuda() for k, v in synthetic.make_batch(B, 101, 256, 3, seed=5, behavior_probs=[0.7, 0.25, 0.05],
                                                      session_mean=sm).items()}
skw = lambda b: dict(session_ids=b["session_ids"], extended_session_ids=b["extended_session_ids"]) if sessions else {}  # noqa: E731
for it in range(2):
    loss, logits = eng.forward(batch["input_ids"], batch["attention_mask"], batch["actions"], labels=batch["labels"], train=True,
                               **skw(batch))
    eng.backward()
torch.cuda.synchronize()
g = eng.flat_g.detach().cpu().contiguous()
step_calls = hashlib.sha256("\n".join(calls).encode()).hexdigest()[:16]
line = (f"{model} B={B} {dt} {mm}: loss {float(loss):.9f} logits {h(logits.float())} grad {h(g)} |g| {float(g.double().norm()):.9f} "
        f"calls {len(calls)} {step_calls}")
if dt == "f32":      # (generation is built for the fp32 engine)
    cat = synthetic.make_catalogue(200, 256)
    eb = synthetic.make_eval_batch(8, 12, cat, 1, 256, 3, min_his=3, seed=5, session_mean=sm)
    act = None if model.startswith("qwen3") else eb["actions"]
    del calls[:]
    _, last = eng.forward(eb["input_ids"], eb["attention_mask"], act, last_row_logits=True, **skw(eb))
    seq, sc = decode.beam_search(eng, eb["input_ids"], eb["attention_mask"], act,
                                 decode.ItemTrie(synthetic.item_tokens(cat, 1, 256).tolist()), 4, 4, **skw(eb))
    torch.cuda.synchronize()
    line += (f" | last_row {h(last.float())} beams {h(seq)} {h(sc)} calls {len(calls)} "
             f"{hashlib.sha256(chr(10).join(calls).encode()).hexdigest()[:16]}")
print(line, flush=True)
