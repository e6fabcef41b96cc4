"""CPU tests of the jet generator of the mask-pattern tests (tests/_jets.py): the patterns are what their names say, the momenta are
on shell with distinct masses, and tile() is the cyclic layout U.tiled_jets always gave."""
import pytest
import torch

import _jets as J
import _util as U
from oracle import lgn_oracle as O


@pytest.mark.parametrize("N", [7, 10, 12, 13, 26, 30, 33, 41, 64, 150])
def test_mask_patterns_are_what_their_names_say(N):
    P = J.mask_patterns(N, torch.Generator().manual_seed(5))
    assert list(P) == J.PATTERNS and all(m.dtype == torch.bool and tuple(m.shape) == (N,) for m in P.values())
    real = {k: m.nonzero().flatten().tolist() for k, m in P.items()}
    assert real["empty"] == [] and real["one_first"] == [0] and real["one_last"] == [N - 1] and real["two_apart"] == [1, N // 2]
    assert len(real["three_random"]) == 3
    assert real["suffix5"] == list(range(N - 5, N))
    assert real["odd"] == list(range(1, N, 2))
    assert real["mod4"] == [i for i in range(N) if i % 4]
    assert real["prefix_minus_one"] == list(range(N - 1)) and real["full"] == list(range(N))
    hole = [i for i in range(N) if i not in real["block_hole"]]
    assert hole == (list(range(8, 16)) if N >= 24 else list(range(N // 3, 2 * N // 3 + 1)))      # N >= 24: groups 2 and 3, whole
    assert hole and hole[0] > 0 and hole[-1] < N - 1, "the hole lies between real rows"
    assert 0 < len(real["random_half"]) < N
    for name in ("odd", "mod4", "block_hole", "random_half"):           # a masked row between real rows
        assert any(not P[name][i] for i in range(real[name][0], real[name][-1])), name


def test_named_batches():
    assert len(J.HOLED) == 11 and len(J.SPARSE) == 7 and set(J.HOLED) | set(J.SPARSE) <= set(J.PATTERNS)
    assert J.SPARSE.count("empty") == 2 and "empty" in J.HOLED and "full" in J.HOLED and "full" not in J.SPARSE
    N = 30
    assert max(int(J.mask_patterns(N, torch.Generator().manual_seed(0))[n].sum()) for n in J.SPARSE) == 5


@pytest.mark.parametrize("N", [7, 30])
def test_pattern_jets_momenta(N):
    p4, labels = J.pattern_jets(N, J.HOLED, 11)
    assert p4.dtype == torch.float64 and labels.dtype == torch.uint8 and tuple(p4.shape) == (11, N, 4) and tuple(labels.shape) == (11, N)
    q4, q_labels = J.pattern_jets(N, J.HOLED, 11)
    assert torch.equal(p4, q4) and torch.equal(labels, q_labels), "same seed, same jets"
    real = labels.bool()
    assert bool((p4[~real] == 0).all()) and bool((p4[real][:, 0] > 0).all())
    full = J.HOLED.index("full")
    assert float(p4.abs().max()) <= 1.0 and abs(float(p4[full].abs().max()) - 1.0) < 1e-15      # normalize_p4_overall_max: per jet
    m2 = O.normsq4(p4[real])
    assert float(m2.min()) > 0 and len(torch.unique(m2)) == m2.numel(), "distinct positive masses"
    m2_full = O.normsq4(p4[full])                                         # m^2 ~ U(0.01, 0.25) before the jet's normalisation
    assert float(m2_full.min() / m2_full.max()) >= 0.04 - 1e-9
    for b, name in enumerate(J.HOLED):
        assert torch.equal(labels[b].bool(), J.mask_patterns(N, torch.Generator().manual_seed(11))[name])


def test_disagree_changes_three_jets_and_no_label():
    p4, labels = J.pattern_jets(30, J.HOLED, 11)
    q4, q_labels = J.disagree(p4, labels, torch.Generator().manual_seed(12))
    assert torch.equal(q_labels, labels) and torch.equal(q4[3:], p4[3:]) and q4.data_ptr() != p4.data_ptr()
    masked0 = ~labels[0].bool()
    assert bool((q4[0][masked0] != 0).all()) and torch.equal(q4[0][~masked0], p4[0][~masked0])
    r1 = labels[1].nonzero().flatten()
    assert torch.equal(q4[1, r1[3]], q4[1, r1[0]]) and int((q4[1] != p4[1]).any(-1).sum()) == 1
    r2 = labels[2].nonzero().flatten()
    assert bool((q4[2, r2[1]] == 0).all()) and int(labels[2, r2[1]]) == 1 and int((q4[2] != p4[2]).any(-1).sum()) == 1


@pytest.mark.parametrize("names", [J.HOLED, J.SPARSE], ids=["holed", "sparse"])
@pytest.mark.parametrize("N", [12, 30, 65])
def test_recon_like_rows(N, names):
    p4, labels = J.pattern_jets(N, names, 11)
    x = J.recon_like(p4, labels, torch.Generator().manual_seed(13))
    assert x.dtype == torch.float64 and tuple(x.shape) == tuple(p4.shape)
    assert torch.equal(x, J.recon_like(p4, labels, torch.Generator().manual_seed(13))), "same generator state, same reconstruction"
    assert not torch.equal(x, J.recon_like(p4, labels, torch.Generator().manual_seed(14)))
    real = labels.bool()
    empty = labels.sum(1) == 0
    assert int(empty.sum()) == names.count("empty") >= 1
    assert bool((x[empty] == 0).all()) and not bool(torch.signbit(x[empty]).any()), "an all-masked jet is +0 on both sides"
    assert bool((p4[empty] == 0).all())
    assert bool((x[~empty] != 0).all()), "no other row holds a zero: a decoder never returns one"
    rel = ((x - p4) / p4)[real]                                          # real rows: within 5 sigma of rel = 0.05, and moved
    assert float(rel.abs().max()) < 0.25 + 1e-12 and float(rel.abs().min()) > 0
    masked = (~real) & (~empty).unsqueeze(1)
    assert float(x[masked].abs().max()) < 5e-3 and float(x[masked].abs().max()) < 0.1 * float(x[real].abs().max())


def test_recon_like_on_disagreeing_labels():
    """The draws do not depend on the labels or the momenta: the disagreeing copy's reconstruction differs from the batch's only where
    the target does, never follows a masked row's stray momenta, and fills the real row of zeros."""
    p4, labels = J.pattern_jets(12, J.HOLED, 11)
    q4, q_labels = J.disagree(p4, labels, torch.Generator().manual_seed(12))
    x, y = (J.recon_like(t, labels, torch.Generator().manual_seed(13)) for t in (p4, q4))
    assert torch.equal(x[3:], y[3:]) and torch.equal(x[0], y[0])
    masked0 = ~labels[0].bool()
    assert float(y[0][masked0].abs().max()) < 5e-3 < float(q4[0][masked0].abs().max())
    zeroed = labels[2].nonzero().flatten()[1]
    assert bool((q4[2, zeroed] == 0).all()) and bool((y[2, zeroed] != 0).all()) and float(y[2, zeroed].abs().max()) < 5e-3
    assert int((x[1] != y[1]).any(-1).sum()) == 1 and int((x[2] != y[2]).any(-1).sum()) == 1


def test_tile_is_the_cyclic_layout_of_tiled_jets():
    p4, labels = J.pattern_jets(12, J.HOLED, 3)
    t4, t_labels, copies = J.tile(p4, labels, 275)
    assert tuple(t4.shape) == (275, 12, 4) and copies.tolist() == [25] * 11
    assert all(torch.equal(t4[b], p4[b % 11]) and torch.equal(t_labels[b], labels[b % 11]) for b in range(275))
    assert J.tile(p4, labels, 30)[2].tolist() == [3] * 8 + [2] * 3
    with pytest.raises(AssertionError):
        J.tile(p4[:10], labels[:10], 40)
    # U.tiled_jets goes through tile(): the batch it always gave
    a4, a_labels, k4, k_labels, a_copies = U.tiled_jets(20, 9, K=7, seed=4)
    s4, s_labels = O.synthetic_jets(7, 9, seed=4, pad=True)
    idx = torch.arange(20) % 7
    assert torch.equal(k4, s4) and torch.equal(k_labels, s_labels) and torch.equal(a4, s4[idx]) and torch.equal(a_labels, s_labels[idx])
    assert a_copies.tolist() == [3, 3, 3, 3, 3, 3, 2] and a4.is_contiguous()
