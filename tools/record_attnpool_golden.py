"""Records tests/golden/g20_attnpool.npz: the REAL reference AttentionPool2d (CLIP/clip/model.py:58-104, imported through
oracle.ref_shim) on the seeded module and inputs of tests/oracle_attnpool.py -- C = 128, heads 2, out 64, S = 3 on 3x3, 5x4 and 2x2 maps,
fp32 on the CPU.  The file holds the state dict, the inputs (channels-last, as the builders make them) and both outputs per map;
tests/test_attnpool_host.py checks the fp64 restatement against it on any machine.  Needs the reference tree: run where it is present
(never on the GPU machine).

    python tools/record_attnpool_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    from oracle import ref_shim
    ref_shim.install()
    from CLIP.clip.model import AttentionPool2d      # the reference's
    import oracle_attnpool as A

    out = {}
    for name in A.SMALL:
        B, C, heads, odim, S, h, w = A.CASES[name]
        sd, x, _, _ = A.case(name)
        m = AttentionPool2d(S, C, heads, odim).float().eval()
        m.load_state_dict({k[len(A.PREFIX) + 1:]: v for k, v in sd.items()})
        with torch.no_grad():
            glob, fmap = m(x.permute(0, 3, 1, 2).contiguous())
        out[f"{name}_x"] = x.numpy()
        out[f"{name}_global"] = glob.contiguous().numpy()
        out[f"{name}_feature_map"] = fmap.contiguous().numpy()
        for k, v in sd.items():                      # one module for the three maps
            assert f"sd_{k}" not in out or np.array_equal(out[f"sd_{k}"], v.numpy())
            out[f"sd_{k}"] = v.numpy()
    path = os.path.join(ROOT, "tests", "golden", "g20_attnpool.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
