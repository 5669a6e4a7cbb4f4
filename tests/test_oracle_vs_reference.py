"""Cross-check against the real reference on inputs that are NOT in the other golden vectors: the oracle and the drop-in
argparse surface are compared with what the reference returned for them, recorded by oracle/gen_golden_live.py in
tests/golden/g12_reference_*.  CPU only; runs anywhere."""
import json
import os

import numpy as np
import torch

from conftest import GOLDEN


def test_argparse_surface_matches_reference():
    from tris_amd.args import get_parser
    ref = json.load(open(os.path.join(GOLDEN, "g12_reference_live.json")))
    assert vars(get_parser().parse_args([])) == ref["args_default"]
    argv = ["--batch_size", "48", "--size", "320", "--negative_samples", "3", "--weight_decay", "0.02", "--distributed",
            "--print-freq", "5", "--backbone", "clip-RN50"]
    assert argv == ref["args_argv"]
    assert vars(get_parser().parse_args(argv)) == ref["args_parsed"]


def test_oracle_matches_live_reference_on_fresh_inputs(golden):
    from oracle import tris_oracle as O
    from tris_amd.utils.shapes import empty_state_dict, tris_state_dict_spec
    from tris_amd.utils.synth import seed_fill, synthetic_batch
    b = synthetic_batch(2, 320, 20, 0, seed=123)
    sd = seed_fill(empty_state_dict(tris_state_dict_spec()), 777)   # = the reference model's state dict after seed_fill(777)
    want = torch.from_numpy(golden("g12_reference_fwd_eval.npz")["fwd_eval"])
    with torch.no_grad():
        got = O.tris_forward(sd, b["img"], b["word_ids"], False)
    assert float((want - got).abs().max()) < 5e-5
    sd = seed_fill(empty_state_dict(tris_state_dict_spec()), 777)
    tr = golden("g12_reference_fwd_train.npz")
    w = [torch.from_numpy(tr[f"fwd_train_{i}"]) for i in range(len(tr.files))]
    with torch.no_grad():
        g = O.tris_forward(sd, b["img"], b["word_ids"], True)
    assert len(g) == len(w)
    for a, c in zip(w, g):
        assert float((a - c).abs().max()) < 5e-5
