"""TEST INFRASTRUCTURE ONLY -- records what the REAL reference returns for the cases of the former live cross-checks
(tests/test_oracle_vs_reference.py, tests/test_dataset.py::test_refer_dataset_matches_live_reference,
tests/test_dropin.py::test_signatures_match_the_live_reference), so that those tests run on any machine:

    python oracle/gen_golden_live.py

It imports the reference through oracle/ref_shim.py (which knows where the reference checkout is) and writes
tests/golden/g12_reference_{fwd_eval,fwd_train,dataset}.npz (model outputs, dataset items) and
tests/golden/g12_reference_live.json (argparse results, caller-facing signatures).  Recorded data only; no reference
source travels.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden")

# the parse_args argv of the argparse case (tests/test_oracle_vs_reference.py)
ARGV = ["--batch_size", "48", "--size", "320", "--negative_samples", "3", "--weight_decay", "0.02", "--distributed",
        "--print-freq", "5", "--backbone", "clip-RN50"]
# the three ReferDataset configurations of tests/test_dataset.py: (split, eval_mode, negative_samples)
DS_CASES = (("train", False, 2), ("val", True, 0), ("train", False, 0))
DS_IMAGES, DS_SEED, DS_SIZE, DS_RNG = 9, 23, 40, 3


def jsonable(v):
    """non-array dataset values (strings, numbers, lists of them) in a comparable form"""
    if isinstance(v, (list, tuple)):
        return [jsonable(x) for x in v]
    if isinstance(v, np.generic):
        return v.item()
    return v


def dataset_items(DS, tf, root):
    """{key: array} of every item of every configuration; non-array values as JSON strings"""
    g = {}
    for c, (split, ev, neg) in enumerate(DS_CASES):
        kw = dict(refer_data_root=root, dataset="refcocog", splitBy="umd", split=split, size=DS_SIZE, max_tokens=20,
                  eval_mode=ev, negative_samples=neg)
        ds = DS(image_transforms=tf(DS_SIZE, train=not ev), **kw)
        g[f"ds{c}_ref_ids"] = np.array(ds.ref_ids)
        np.random.seed(DS_RNG)
        for i in range(len(ds)):
            for part, d in zip("st", ds[i]):
                for k, v in d.items():
                    key = f"ds{c}_{i}_{part}_{k}"
                    if torch.is_tensor(v):
                        g[key] = v.numpy()
                    elif isinstance(v, np.ndarray):
                        g[key] = v
                    else:
                        g[key + "__json"] = np.array(json.dumps(jsonable(v)))
    return g


def main():
    from oracle import ref_shim
    from oracle import tris_oracle as O
    from tris_amd.utils.shapes import empty_state_dict, tris_state_dict_spec
    from tris_amd.utils.synth import make_mini_refer, seed_fill, synthetic_batch
    g, js = {}, {}

    # argparse surface
    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_args", os.path.join(ref_shim.REF_ROOT, "args.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    js["args_default"] = vars(mod.get_parser().parse_args([]))
    js["args_argv"] = ARGV
    js["args_parsed"] = vars(mod.get_parser().parse_args(ARGV))

    # TRIS forward on fresh inputs, eval and train mode
    torch.manual_seed(0)
    ref = ref_shim.make_tris()
    seed_fill(ref.state_dict(), 777)
    sd = seed_fill(empty_state_dict(tris_state_dict_spec()), 777)
    assert list(sd) == list(ref.state_dict()) and all(torch.equal(sd[k], v) for k, v in ref.state_dict().items()), \
        "the seed-filled spec no longer reproduces the reference's seed-filled state dict"
    b = synthetic_batch(2, 320, 20, 0, seed=123)
    with torch.no_grad():
        ref.eval()
        g["fwd_eval"] = ref(b["img"], b["word_ids"]).numpy()
        ref.train()
        for i, t in enumerate(ref(b["img"], b["word_ids"])):
            g[f"fwd_train_{i}"] = t.numpy()
    print("oracle deviation (eval):", float((O.tris_forward(sd, b["img"], b["word_ids"], False) -
                                             torch.from_numpy(g["fwd_eval"])).abs().max()))

    # ReferDataset items on the synthetic mini dataset, the real BPE tokenizer
    RefDS, ref_tf = ref_shim.install_dataset()
    root = make_mini_refer(tempfile.mkdtemp(), n_images=DS_IMAGES, seed=DS_SEED)
    g.update(dataset_items(RefDS, ref_tf, root))

    # caller-facing signatures under the reference's own import names (tests/_dropin_probe.py, fresh process)
    r = subprocess.run([sys.executable, "-B", os.path.join(ROOT, "tests", "_dropin_probe.py"), "reference"],
                       capture_output=True, text=True, cwd=ROOT, check=True)
    js["signatures"] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("PROBE ")][-1][6:])

    # three archives, each under the size limit of a committed file
    for name, keep in (("fwd_eval", lambda k: k == "fwd_eval"), ("fwd_train", lambda k: k.startswith("fwd_train_")),
                       ("dataset", lambda k: k.startswith("ds"))):
        f = os.path.join(OUT, f"g12_reference_{name}.npz")
        np.savez_compressed(f, **{k: v for k, v in g.items() if keep(k)})
        print(os.path.basename(f), os.path.getsize(f), "bytes")
    with open(os.path.join(OUT, "g12_reference_live.json"), "w") as f:
        json.dump(js, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
