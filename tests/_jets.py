"""Jets with holes, sparse jets and batches whose labels and momenta disagree: the inputs of the mask-pattern tests.

O.synthetic_jets(..., pad=True) -- what every other test feeds to a mask-reading kernel -- puts the real particles first, keeps at least
min(10, N) of them, and gives every particle m^2 = 1e-6.  The jets here carry one named mask pattern each, with isotropic momenta and
DISTINCT masses: with equal masses the two particles of a two-particle jet carry the same scalar features in exact arithmetic, min / max
pooling ties (U.assert_live: gap 8e-16) and the oracle disagrees with itself by 2.5e-2 in the reconstruction when the particles are
listed in reverse.  With m^2 ~ U(0.01, 0.25) the oracle against itself (particles and labels of every jet reversed, live weights, SPARSE
and HOLED at N = 13 .. 65, maxdim 2 and 3) differs by at most 2.7e-15 per jet in the reconstruction and 1.9e-13 in a gradient tensor.

tests/golden/gen_golden.py restates pattern_jets / disagree with the reference's normalize_p4 for the g28 fixtures; the two must stay
the same recipe (test_oracle_golden.py compares the stored inputs with what this module gives)."""
import torch

PATTERNS = ["empty", "one_first", "one_last", "two_apart", "three_random", "suffix5", "odd", "mod4", "block_hole", "random_half",
            "prefix_minus_one", "full"]

# the gradients of SPARSE come from sparse jets alone (in a mixed batch a full jet's gradient is 1e3 times theirs)
SPARSE = ["empty", "one_first", "one_last", "two_apart", "three_random", "suffix5", "empty"]
# K = 11 distinct jets: odd, so that tile() lands a kernel that reads a neighbour's jet at a power-of-two offset on other data
HOLED = ["odd", "mod4", "block_hole", "random_half", "prefix_minus_one", "suffix5", "full", "empty", "one_last", "two_apart",
         "three_random"]


def mask_patterns(N, g):
    """Ordered {name: bool (N,)} of the real rows; g: the torch.Generator the two random patterns draw from (three_random first)."""
    ar = torch.arange(N)
    rows = lambda *idx: torch.zeros(N, dtype=torch.bool).index_fill_(0, torch.tensor(idx, dtype=torch.long), True)   # noqa: E731
    lo, hi = (8, 15) if N >= 24 else (N // 3, 2 * N // 3)          # block_hole masks rows lo .. hi: two whole groups of four for N >= 24
    P = {"empty": rows(),
         "one_first": rows(0),
         "one_last": rows(N - 1),
         "two_apart": rows(1, N // 2),
         "three_random": rows(*torch.randperm(N, generator=g)[:3].tolist()),
         "suffix5": ar >= N - min(5, N),
         "odd": ar % 2 == 1,
         "mod4": ar % 4 != 0,
         "block_hole": (ar < lo) | (ar > hi),
         "random_half": torch.rand(N, generator=g) < 0.5,
         "prefix_minus_one": ar < N - 1,
         "full": torch.ones(N, dtype=torch.bool)}
    assert list(P) == PATTERNS
    return P


def pattern_jets(N, names, seed):
    """(p4 (B, N, 4) float64, labels (B, N) uint8): jet b carries mask pattern names[b].  p3 ~ N(0, 1), m^2 ~ U(0.01, 0.25) per
    particle, E = sqrt(|p3|^2 + m^2), O.normalize_p4_overall_max (per jet, over all N rows), then the masked rows multiplied to zero."""
    from oracle import lgn_oracle as O
    g = torch.Generator().manual_seed(seed)
    P = mask_patterns(N, g)
    labels = torch.stack([P[n] for n in names]).to(torch.uint8)
    B = len(names)
    p3 = torch.randn(B, N, 3, dtype=torch.float64, generator=g)
    m2 = 0.01 + 0.24 * torch.rand(B, N, 1, dtype=torch.float64, generator=g)
    e = torch.sqrt((p3 * p3).sum(-1, keepdim=True) + m2)
    p4 = O.normalize_p4_overall_max(torch.cat([e, p3], -1)) * labels.unsqueeze(-1).to(torch.float64)
    return p4, labels


def disagree(p4, labels, g):
    """A copy of the batch in which labels and momenta disagree (the reference takes the mask from data['labels'], not from p4:
    lgn_encoder.py:386-403).  Jet 0: the masked rows get fresh non-zero momenta, labels still 0.  Jet 1: its fourth real row becomes a
    copy of its first -- exact duplicates, so the `norms != 0` edge mask fires off the diagonal.  Jet 2: its second real row is zeroed,
    label still 1.  Returns (p4, labels); g: the torch.Generator of the fresh momenta."""
    q, lab = p4.clone(), labels.clone()
    N = q.shape[1]
    fresh = 0.2 * torch.randn(N, 3, dtype=torch.float64, generator=g)
    fresh = torch.cat([torch.sqrt((fresh * fresh).sum(-1, keepdim=True) + 0.05), fresh], -1)
    q[0] = torch.where(lab[0].bool().unsqueeze(-1), q[0], fresh)
    real1, real2 = lab[1].nonzero().flatten(), lab[2].nonzero().flatten()
    assert int((~lab[0].bool()).sum()) >= 1 and len(real1) >= 4 and len(real2) >= 2, "the first three jets are too sparse to disagree"
    q[1, real1[3]] = q[1, real1[0]]
    q[2, real2[1]] = 0
    return q, lab


def recon_like(p4, labels, g, rel=0.05):
    """A stand-in for a decoder's reconstruction of the target (p4, labels), for the calls that take (reconstruction, target) without
    the networks.  A row that is real by its label AND carries momenta: every component times 1 + rel N(0, 1).  Every other row
    (masked, or a real row of zeros as `disagree` makes one): 1e-3 N(0, 1) per component -- a decoder never returns zeros there, and
    never returns the target's stray momenta of a masked row either.  A jet without a real label: exactly zero, as the decoder returns
    it (g28).  g: the torch.Generator; the draws do not depend on the labels, so a batch and its `disagree` copy share them."""
    noise = torch.randn(p4.shape, dtype=torch.float64, generator=g)
    small = 1e-3 * torch.randn(p4.shape, dtype=torch.float64, generator=g)
    real = labels.bool() & (p4 != 0).any(-1)
    x = torch.where(real.unsqueeze(-1), p4 * (1.0 + rel * noise), small)
    return torch.where((labels.sum(1) > 0).view(-1, 1, 1), x, torch.zeros_like(x))


def tile(p4, labels, B):
    """B jets made of the K given ones laid out cyclically (jet b = given jet b % K; K odd, so coprime to every power of two).
    Returns (p4 (B, N, 4), labels (B, N), copies (K,): how often each given jet occurs).  A loss that is a sum over jets is then
    sum_k copies_k term_k of the K jets, gradient included."""
    K = p4.shape[0]
    assert K % 2 == 1, "an even number of distinct jets shares a factor with the kernels' power-of-two strides"
    idx = torch.arange(B) % K
    return p4[idx].contiguous(), labels[idx].contiguous(), torch.bincount(idx, minlength=K)
