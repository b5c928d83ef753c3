#!/usr/bin/env python3
"""Golden fixture for the weight-decay rule: the parameter names of the REAL reference ``Qwen3MultiWithTemperature``
(imported through the shims of ``oracle/_ref_loader.py``, build container only) at a small configuration (5 layers, all
sparse, cross attention in layer 4, 3 behaviours, V = 49) and, for each, whether HF ``Trainer.get_decay_parameter_names``
puts it in the weight-decay group.  ``tests/test_host_logic.py`` checks ``oracle.qwen3multi_oracle.is_no_decay``
against it.

Usage:  python oracle/make_golden_no_decay.py        (writes tests/golden/no_decay.npz)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gamer_amd import synthetic  # noqa: E402
from oracle import _ref_loader  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "no_decay.npz")
SPEC = dict(num_behavior=3, vocab_size=49, codebook=8, num_hidden_layers=5, sparse_layers_decoder=[0, 1, 2, 3, 4],
            cross_attention_decoder=[4])


def main():
    import transformers
    from transformers import Trainer
    Model, Cfg = _ref_loader.load_reference_classes()
    cfg = _ref_loader.reference_config(Cfg, SPEC["num_behavior"], SPEC["vocab_size"],
                                       synthetic.behavior_maps(SPEC["codebook"], SPEC["num_behavior"]),
                                       num_hidden_layers=SPEC["num_hidden_layers"],
                                       sparse_layers_decoder=SPEC["sparse_layers_decoder"],
                                       cross_attention_decoder=SPEC["cross_attention_decoder"])
    model = Model(cfg)
    decay = set(Trainer.get_decay_parameter_names(None, model))
    names = [n for n, _ in model.named_parameters()]
    meta = dict(spec=SPEC, generator=dict(reference="wzf2000/GAMER", transformers=transformers.__version__,
                                          rule="transformers.Trainer.get_decay_parameter_names"))
    flags = np.array([n in decay for n in names])
    np.savez_compressed(OUT, names=np.array(names), decay=flags, meta_json=np.array(json.dumps(meta)))
    print("wrote", OUT, os.path.getsize(OUT), f"({len(names)} parameters, {int((~flags).sum())} without decay)")


if __name__ == "__main__":
    main()
