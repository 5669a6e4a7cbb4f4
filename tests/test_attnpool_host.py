"""CPU checks of CLIP's attention pooling (no GPU): the folding algebra in fp64, the fp64 restatement against the recorded reference
module (tests/golden/g20_attnpool.npz, tools/record_attnpool_golden.py), the argument contracts of the two ops and the weight-concat
cache of AttentionPool2d."""
import pytest
import torch

import oracle_attnpool as A


@pytest.mark.parametrize("name", list(A.CASES))
def test_folded_form_equals_token0_of_the_full_form_in_fp64(name):
    sd, x, heads, S = A.case(name)
    sd64, x64 = A.to(sd, torch.float64), x.double()
    glob, _ = A.full(sd64, x64, heads, S)
    got = A.folded(sd64, x64, heads, S)
    e = float((got - glob).abs().max() / glob.abs().max())
    print(f"{name}: folded vs full, fp64: {e:.3g} of the output maximum")
    assert e < 1e-12


@pytest.mark.parametrize("name", A.SMALL)
def test_fp64_restatement_matches_the_recorded_reference_module(golden, name):
    g = golden("g20_attnpool.npz")
    sd, x, heads, S = A.case(name)
    for k, v in sd.items():                                   # the builders still make what was recorded
        assert torch.equal(v, torch.from_numpy(g[f"sd_{k}"])), k
    assert torch.equal(x, torch.from_numpy(g[f"{name}_x"]))
    glob, fmap = A.full(A.to(sd, torch.float64), x.double(), heads, S)
    ref_g, ref_f = torch.from_numpy(g[f"{name}_global"]).double(), torch.from_numpy(g[f"{name}_feature_map"]).double()
    assert ref_f.shape == fmap.shape and 0.3 < float(ref_g.abs().max()) < 10.0   # unit-scale outputs: the tolerance is absolute
    eg, ef = float((glob - ref_g).abs().max()), float((fmap - ref_f).abs().max())
    print(f"{name}: restatement vs recorded reference: global {eg:.3g}, feature_map {ef:.3g}")
    assert eg < 5e-6 and ef < 5e-6
    assert float((A.folded(A.to(sd, torch.float64), x.double(), heads, S) - ref_g).abs().max()) < 5e-6


def test_argument_contracts_raise_by_name():
    from tris_amd import ops
    pos = torch.zeros(10, 128)
    with pytest.raises(ValueError, match=r"attnpool_tokens.*1025"):
        ops.attnpool_tokens(torch.zeros(1, 32, 33, 128), pos, 3)            # L = 1057
    with pytest.raises(ValueError, match=r"attnpool_tokens.*C % 4"):
        ops.attnpool_tokens(torch.zeros(1, 3, 3, 126), torch.zeros(10, 126), 3)
    with pytest.raises(ValueError, match=r"attnpool_tokens.*pos"):
        ops.attnpool_tokens(torch.zeros(1, 3, 3, 128), pos, 4)
    with pytest.raises(ValueError, match=r"attnpool_pool.*1025"):
        ops.attnpool_pool(torch.zeros(1, 1026, 128), torch.zeros(1, 2, 128), 0.125)
    with pytest.raises(ValueError, match=r"attnpool_pool.*C % 4"):
        ops.attnpool_pool(torch.zeros(1, 10, 126), torch.zeros(1, 2, 126), 0.125)
    with pytest.raises(ValueError, match=r"attnpool_pool"):
        ops.attnpool_pool(torch.zeros(1, 10, 128), torch.zeros(2, 2, 128), 0.125)
    x = torch.zeros(1, 3, 3, 128, requires_grad=True)
    with pytest.raises(NotImplementedError, match="attnpool_tokens"):
        ops.attnpool_tokens(x, pos, 3)
    with pytest.raises(NotImplementedError, match="attnpool_tokens"):
        ops.attnpool_tokens(x.detach(), pos.clone().requires_grad_(), 3)
    with pytest.raises(NotImplementedError, match="attnpool_pool"):
        ops.attnpool_pool(torch.zeros(1, 10, 128, requires_grad=True), torch.zeros(1, 2, 128), 0.125)
    with pytest.raises(NotImplementedError, match="attnpool_pool"):
        ops.attnpool_pool(torch.zeros(1, 10, 128), torch.zeros(1, 2, 128, requires_grad=True), 0.125)


def test_both_ops_refuse_the_cpu():
    from tris_amd import ops
    with pytest.raises(ops.NoGpuError):
        ops.attnpool_tokens(torch.zeros(1, 3, 3, 128), torch.zeros(10, 128), 3)
    with pytest.raises(ops.NoGpuError):
        ops.attnpool_pool(torch.zeros(1, 10, 128), torch.zeros(1, 2, 128), 0.125)
    with torch.no_grad():                                      # grad-requiring inputs are fine where grad mode is off
        with pytest.raises(ops.NoGpuError):
            ops.attnpool_tokens(torch.zeros(1, 3, 3, 128, requires_grad=True), torch.zeros(10, 128), 3)


def test_module_refuses_the_cpu_and_a_gradient():
    from tris_amd import ops
    from tris_amd.CLIP.clip.model import AttentionPool2d
    m = AttentionPool2d(3, 128, 2, 64)
    assert all(getattr(p, "_tris_no_grad_path", False) for p in m.parameters())
    with pytest.raises(ops.NoGpuError):
        m(torch.zeros(1, 128, 3, 3))
    with pytest.raises(ops.NoGpuError):
        m(torch.zeros(1, 3, 3, 128), global_only=True)
    with pytest.raises(NotImplementedError, match="AttentionPool2d"):
        m(torch.zeros(1, 128, 3, 3, requires_grad=True))
    with pytest.raises(ValueError, match="AttentionPool2d"):
        m(torch.zeros(1, 64, 3, 3))


def test_weight_concat_cache_follows_the_parameters():
    from tris_amd.CLIP.clip.model import AttentionPool2d
    m = AttentionPool2d(3, 128, 2, 64)
    w, b = m._qkv()
    assert tuple(w.shape) == (384, 128) and tuple(b.shape) == (384,)
    assert torch.equal(w[128:256], m.k_proj.weight) and torch.equal(b[256:], m.v_proj.bias)
    assert m._qkv()[0] is w and m._qkv()[1] is b               # cached: nothing rebuilt
    with torch.no_grad():
        m.k_proj.weight.mul_(2.0)                              # in-place update (an optimiser step): the version moves
    w2, _ = m._qkv()
    assert w2 is not w and torch.equal(w2[128:256], m.k_proj.weight) and torch.equal(w2[:128], w[:128])
    with torch.no_grad():
        m.v_proj.bias.add_(1.0)
    assert torch.equal(m._qkv()[1][256:], m.v_proj.bias)
    m.q_proj.weight.data = m.q_proj.weight.data.clone() + 1.0  # new storage, version unchanged
    assert torch.equal(m._qkv()[0][:128], m.q_proj.weight)
    assert "_qkv_cat" not in m.state_dict() and len(m.state_dict()) == 9
