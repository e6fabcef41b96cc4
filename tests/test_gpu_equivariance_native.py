"""The native equivariance test (lgn.equivariance, csrc/equivariance.hip) on the GPU.

1. transform_jets against a np.longdouble product; 2. rep_deviation against a np.longdouble restatement of rotate_rep plus the five
reductions, with tolerances computed from the test's own inputs (rounding bound of an n-term sum in any order plus the 2d-term
rotation); 3. the native lgn_tests on the g1 / g2 weights and the jets of g8_harness.npz against every assertion
tests/test_gpu_equivariance.py makes of the Python harness, with its numbers unchanged."""
import numpy as np
import pytest
import torch

import _util as U

pytestmark = pytest.mark.gpu

L = np.longdouble
EPS = 2.0 ** -53
# d = 1, 3, 4, 9 (and the second d = 3 irrep): every representation dimension up to maxdim 3
IRREPS = ((0, 0), (2, 0), (1, 1), (2, 2), (0, 2))


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def transforms():
    """A rotation about x, a rotation about z and a boost about y (alpha = 2): the planar D of every irrep and the Cartesian R."""
    from lgn.cg_lib import CGDict
    from lgn.models.autotest.lgn_tests import _angles, cartesian_lorentz, lorentz_D
    cg = CGDict(maxdim=3)
    angs = [_angles("rot", 0.7, "x"), _angles("rot", 1.9, "z"), _angles("boost", 2.0, "y")]
    D = {w: torch.stack([lorentz_D(w, *ang, cg) for ang in angs]) for w in IRREPS}                  # (3, 2, d, d)
    R = torch.stack([cartesian_lorentz(lorentz_D((1, 1), *ang, cg)) for ang in angs])                # (3, 4, 4)
    for w in IRREPS[1:]:
        assert (D[w][:, 0].abs().amax((1, 2)) > 0.1).all() and D[w][:, 1].abs().max() > 0.1, w       # real AND imaginary parts at work
    return {"cg": cg, "angs": angs, "D": D, "R": R}


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. transform_jets
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_perm", [False, True])
def test_transform_jets_vs_longdouble(dev, transforms, with_perm):
    from lgn.equivariance import transform_jets
    rng = np.random.default_rng(11)
    B, n, K = 3, 5, 2
    p4, sc, R = rng.normal(size=(B, n, 4)) * 50.0, rng.normal(size=(B, n, K)), transforms["R"].numpy()
    perm = np.stack([rng.permutation(n) for _ in range(B)]) if with_perm else None
    src = np.stack([p4[b, perm[b]] for b in range(B)]) if with_perm else p4
    src_sc = np.stack([sc[b, perm[b]] for b in range(B)]) if with_perm else sc
    perm_d = torch.from_numpy(perm).to(dev) if with_perm else None

    out, sc_out = transform_jets(torch.from_numpy(p4).to(dev), torch.from_numpy(R).to(dev), perm_d, torch.from_numpy(sc).to(dev))
    assert tuple(out.shape) == (3, B, n, 4) and tuple(sc_out.shape) == (3, B, n, K)
    ref = np.einsum("bnk,tka->tbna", src.astype(L), R.astype(L))
    bound = 4 * EPS * np.einsum("bnk,tka->tbna", np.abs(src), np.abs(R))
    err = np.abs(out.cpu().numpy().astype(L) - ref)
    print("transform_jets: max err / bound", float((err / bound).max()))
    assert (err <= bound).all()
    assert np.array_equal(sc_out.cpu().numpy(), np.broadcast_to(src_sc, (3, B, n, K)))
    only = transform_jets(torch.from_numpy(p4).to(dev), torch.from_numpy(R).to(dev), perm_d)          # without scalars: one tensor
    assert torch.equal(only, out)
    same = transform_jets(torch.from_numpy(p4).to(dev), torch.eye(4, device=dev, dtype=torch.float64), perm_d)
    assert tuple(same.shape) == (1, B, n, 4) and np.array_equal(same[0].cpu().numpy(), src)           # R = I: the gathered input, bitwise


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. rep_deviation
# ---------------------------------------------------------------------------------------------------------------------------------
def rotate_longdouble(b, D):
    """rotate_rep in np.longdouble: b (2, B, N, C, d), D (2, d, d) -> b' (2, B, N, C, d), and the magnitude sum |b| |D| behind it."""
    br, bi, Dr, Di = b[0].astype(L), b[1].astype(L), D[0].astype(L), D[1].astype(L)
    rot = np.stack([br @ Dr + bi @ Di, -(br @ Di) + bi @ Dr])
    mag = np.stack([np.abs(br) @ np.abs(Dr) + np.abs(bi) @ np.abs(Di), np.abs(br) @ np.abs(Di) + np.abs(bi) @ np.abs(Dr)])
    return rot, mag


def restate(a, b, D, perm=None):
    """The five reductions of every t in np.longdouble and their tolerances: a (2, T B, N, C, d), b (2, B, N, C, d), D (T, 2, d, d)."""
    T, B, d = D.shape[0], b.shape[1], b.shape[-1]
    if perm is not None:
        b = np.stack([b[:, i, perm[i]] for i in range(B)], 1)
    ref, tol = np.zeros((T, 5), L), np.zeros((T, 5), L)
    for t in range(T):
        rot, mag = rotate_longdouble(b, D[t])
        at = a[:, t * B:(t + 1) * B].astype(L)
        diff, size = at - rot, np.abs(at) + mag
        ref[t] = [diff.sum(), rot.sum(), np.abs(diff).max(), np.abs(rot).max(), np.abs(diff / (rot + L(1e-16))).max()]
        t_sum, t_max = (diff.size + 2 * d + 4) * EPS * size.sum(), (2 * d + 4) * EPS * size.max()
        tol[t] = [t_sum, t_sum, t_max, t_max, t_max / np.abs(rot + L(1e-16)).min()]
    return ref, tol


def make_case(transforms, B, n, channels, seed, perm=None):
    """Random b of every irrep together; a = b' + 1e-3 |b'| u, u uniform in (0.5, 1): deviations well away from rounding noise.
    With perm, b' is the rotation of b read at particle perm[b][n]."""
    rng = np.random.default_rng(seed)
    T = 3
    a, b, D = [], [], []
    for w, c in zip(IRREPS, channels):
        Dw = transforms["D"][w].numpy()
        d = Dw.shape[-1]
        bw = rng.normal(size=(2, B, n, c, d))
        moved = bw if perm is None else np.stack([bw[:, i, perm[i]] for i in range(B)], 1)
        rot = np.concatenate([rotate_longdouble(moved, Dw[t])[0].astype(np.float64) for t in range(T)], 1)
        a.append(rot + 1e-3 * np.abs(rot) * rng.uniform(0.5, 1.0, size=rot.shape))
        b.append(bw), D.append(Dw)
    return a, b, D


def to_dev(xs, dev):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in xs]


def check(stats, a, b, D, perm=None, what=""):
    stats = stats.cpu().numpy()
    for p, (ap, bp, Dp) in enumerate(zip(a, b, D)):
        ref, tol = restate(ap, bp, Dp, perm)
        err = np.abs(stats[p].astype(L) - ref)
        print(f"{what} part {p} d = {bp.shape[-1]}: max err / tol per statistic", [float(x) for x in (err / tol).max(0)])
        assert (err <= tol).all(), (what, p, err, tol)
        assert (ref[:, 4] > 4e-4).all() and (ref[:, 4] < 1.1e-3).all()           # the planted deviation is what is measured


# B = 1, N = 5 with C in {2, 3}; and rows per (part, t) = two tiles + three (B N C = 5 * 103 * 1 = 515 = 2 * 256 + 3), the last part
# twice that (four tiles and six rows): the cross-workgroup stage and partial tiles
SHAPES = {"small": (1, 5, (2, 3, 2, 3, 2)), "tiles": (5, 103, (1, 1, 1, 1, 2))}


@pytest.fixture(scope="module", params=list(SHAPES))
def case(request, transforms, dev):
    from lgn import _native as N
    from lgn.equivariance import rep_deviation
    B, n, channels = SHAPES[request.param]
    if request.param == "tiles":
        assert B * n * channels[0] == 2 * N.EQUI_TILE + 3
    a, b, D = make_case(transforms, B, n, channels, seed=5)
    ad, bd, Dd = to_dev(a, dev), to_dev(b, dev), to_dev(D, dev)
    return {"name": request.param, "B": B, "n": n, "a": a, "b": b, "D": D, "ad": ad, "bd": bd, "Dd": Dd, "stats": rep_deviation(ad, bd, Dd)}


def test_rep_deviation_vs_longdouble(case):
    assert tuple(case["stats"].shape) == (len(IRREPS), 3, 5)
    check(case["stats"], case["a"], case["b"], case["D"], what=case["name"])


def test_rep_deviation_same_bits_twice(case):
    from lgn.equivariance import rep_deviation
    again = rep_deviation(case["ad"], case["bd"], case["Dd"])
    assert torch.equal(again.view(torch.int64), case["stats"].view(torch.int64))


def test_rep_deviation_of_the_harness_rotation_is_zero(case, transforms, dev):
    """a = the Python harness's fp64 rotate_rep(b): max|a - b'| is rounding, within the bound of zero (conj / non-conj mix-up: O(1))."""
    from lgn.equivariance import MAX_DIFF, rep_deviation
    from lgn.models.autotest.lgn_tests import rotate_rep
    rot = [rotate_rep({w: torch.from_numpy(bw) for w, bw in zip(IRREPS, case["b"])}, *ang, transforms["cg"]) for ang in transforms["angs"]]
    a = [torch.cat([r[w] for r in rot], 1).numpy() for w in IRREPS]
    stats = rep_deviation(to_dev(a, dev), case["bd"], case["Dd"]).cpu().numpy()
    for p, (ap, bp, Dp) in enumerate(zip(a, case["b"], case["D"])):
        _, tol = restate(ap, bp, Dp)
        print(f"harness rotation part {p}: max|a - b'|", stats[p, :, MAX_DIFF], "bound", [float(x) for x in tol[:, MAX_DIFF]])
        assert (stats[p, :, MAX_DIFF] <= tol[:, MAX_DIFF]).all()


def test_rep_deviation_nan_stays_in_its_block(case, dev):
    """torch's mean and max keep a NaN.  One in D[part][t] reaches b' of block (part, t) alone: exactly its five numbers are NaN.  One
    in a reaches what a enters -- sum(a - b'), max|a - b'| and the relative max -- and leaves
    sum(b') and max|b'| as they were, as (a - b).mean() and b.abs().max() do."""
    from lgn.equivariance import MAX_B, SUM_B, rep_deviation
    B = case["B"]
    part, t = 3, 1

    def nan_where(stats):
        return torch.isnan(stats).cpu()

    def same_bits(x, y):
        return torch.equal(x.view(torch.int64), y.view(torch.int64))

    D = [x.copy() for x in case["D"]]
    D[part][t, 1, -1, -1] = np.nan
    stats = rep_deviation(case["ad"], case["bd"], to_dev(D, dev))
    want = torch.zeros(len(IRREPS), 3, 5, dtype=torch.bool)
    want[part, t] = True
    assert torch.equal(nan_where(stats), want)
    keep = ~want.to(stats.device)
    assert same_bits(stats[keep], case["stats"][keep])

    a = [x.copy() for x in case["a"]]
    a[part][1, t * B + B - 1, -1, -1, -1] = np.nan                    # the last element of block (part 3, t = 1), imaginary plane
    stats = rep_deviation(to_dev(a, dev), case["bd"], case["Dd"])
    want[part, t, SUM_B] = want[part, t, MAX_B] = False
    assert torch.equal(nan_where(stats), want)
    keep = ~want.to(stats.device)
    assert same_bits(stats[keep], case["stats"][keep])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_rep_deviation_with_perm(transforms, dev, shape):
    """With perm: the restatement with b gathered (a is made from the gathered b, so the planted deviation is again what is
    measured; read without perm, or with another one, the deviations are of order 1).  Every part has the same N, as the call asks."""
    from lgn.equivariance import MAX_REL, rep_deviation
    rng = np.random.default_rng(3)
    B, n, channels = SHAPES[shape]
    perm = np.stack([rng.permutation(n) for _ in range(B)])
    assert (perm != np.arange(n)).any()
    a, b, D = make_case(transforms, B, n, channels, seed=6, perm=perm)
    ad, bd, Dd = to_dev(a, dev), to_dev(b, dev), to_dev(D, dev)
    check(rep_deviation(ad, bd, Dd, perm=torch.from_numpy(perm).to(dev)), a, b, D, perm, what="perm " + shape)
    assert (rep_deviation(ad, bd, Dd)[:, :, MAX_REL] > 1e-2).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. end to end: the assertions of tests/test_gpu_equivariance.py on the native harness
# ---------------------------------------------------------------------------------------------------------------------------------
CASES = {"g1": ("g1_e2e_maxdim2.npz", 2), "g2": ("g2_e2e_maxdim3.npz", 3)}


def modules(tag, dev):
    import __graft_entry__ as G
    name, maxdim = CASES[tag]
    z, h = U.load(name), U.load("g8_harness.npz")
    m = U.meta(z)
    enc, dec = G._models(m["N"], m["ch_enc"], m["ch_dec"], dev, seed=m["seed"], maxdim=maxdim)
    enc.load_state_dict(U.params_from(z, "enc")); dec.load_state_dict(U.params_from(z, "dec"))
    p4, labels = torch.from_numpy(h[f"{tag}.p4"]), torch.from_numpy(h[f"{tag}.labels"])
    assert tuple(p4.shape) == (6, 30, 4)
    return enc, dec, [{"p4": p4.clone(), "labels": labels.clone()}], h, maxdim


def assert_tables(tag, maxdim, res, h):
    """tests/test_gpu_equivariance.py, its thresholds and bounds unchanged (their reasons are written there)."""
    from lgn.models.autotest import check_equivariance
    gam = np.asarray(res["gammas"])
    np.testing.assert_allclose(gam, h[f"{tag}.gammas"], rtol=1e-13)
    if maxdim == 2:
        bad = check_equivariance(res)
        assert not bad, "native harness violates the equivariance thresholds:\n" + "\n".join(bad)
    else:
        sub = dict(res)
        keep = [i for i, g in enumerate(gam) if g <= 1000.0]
        sub["gammas"] = [res["gammas"][i] for i in keep]
        sub["boost_dev_output"] = [res["boost_dev_output"][i] for i in keep]
        bad = check_equivariance(sub, {"rotation": 5e-9, "boost_gamma_le_10": 1e-8, "boost_gamma_le_1000": 1e-5})
        assert not bad, "native harness (maxdim 3) violates the equivariance thresholds:\n" + "\n".join(bad)
    irreps = [(0, 0), (1, 1)]
    floor = 2e-13 if maxdim == 2 else 1e-10
    for kind, xs in (("rot", np.ones(26)), ("boost", gam)):
        ref = h[f"{tag}.{kind}_dev_output"]
        assert len(res[f"{kind}_dev_output"]) == 26
        for row, (a, gm) in enumerate(zip(res[f"{kind}_dev_output"], xs)):
            for col, irrep in enumerate(irreps):
                bound = max(20 * max(ref[row][col], floor), floor + (5e-14 if maxdim == 2 else 1e-12) * float(gm) ** 2)
                assert a[irrep] <= bound, f"{tag} {kind} output {irrep} gamma={float(gm):.4g}: native {a[irrep]:.2e} vs reference {ref[row][col]:.2e}"
        ref_i = h[f"{tag}.{kind}_dev_internal"]
        assert len(res[f"{kind}_dev_internal"][0]) == ref_i.shape[1]
        for row, (per_alpha, gm) in enumerate(zip(res[f"{kind}_dev_internal"], xs)):
            for layer, d in enumerate(per_alpha):
                for col, irrep in enumerate(irreps):
                    bound = max(50 * max(ref_i[row][layer][col], floor), 100 * (floor + 1e-12 * float(gm) ** 2))
                    assert d[irrep] <= bound, f"{tag} {kind} internal layer {layer} {irrep} gamma={float(gm):.4g}: {d[irrep]:.2e} vs {ref_i[row][layer][col]:.2e}"
        for per_alpha, gm in zip(res[f"{kind}_dev_internal_all"], xs):
            for layer, d in enumerate(per_alpha):
                for irrep, v in d.items():
                    if kind == "rot":
                        assert v <= 2e-7, f"{tag} rotation internal layer {layer} {irrep}: {v:.2e}"
                    elif gm <= 1000.0:
                        lim = 1e-7 * max(1.0, float(gm) ** 2) if layer == 0 else 2e-7 + 1e-10 * float(gm) ** 2
                        assert v <= lim, f"{tag} boost internal layer {layer} {irrep} gamma={float(gm):.3g}: {v:.2e}"
    if maxdim == 3:
        seen = {irrep for per_alpha in res["rot_dev_internal_all"] for d in per_alpha for irrep in d}
        assert {(2, 0), (0, 2), (2, 2)} <= seen, f"the maxdim-3 internal features were not all checked: {sorted(seen)}"
    assert max(res["perm_invariance_dev_output"].values()) <= 1e-10
    print(tag, "max rot dev native harness / reference:", max(max(d[w] for w in irreps) for d in res["rot_dev_output"]), h[f"{tag}.rot_dev_output"].max())
    print(tag, "max boost dev (gamma <= 1000) native harness / reference:",
          max(max(d[w] for w in irreps) for d, g in zip(res["boost_dev_output"], gam) if g <= 1000), h[f"{tag}.boost_dev_output"][gam <= 1000].max())


@pytest.mark.parametrize("tag, max_jets", [("g1", 512), ("g2", 512), ("g1", 30)])
def test_native_harness_vs_reference_tables(dev, tag, max_jets):
    """max_jets = 30: chunks of five angles (six forwards of 30 jets, the last of 6) instead of one forward of 156 jets."""
    from lgn.models.autotest import lgn_tests_native
    enc, dec, loader, h, maxdim = modules(tag, dev)
    res = lgn_tests_native(None, enc, dec, loader, unit="TeV", irreps="all", max_jets=max_jets)
    assert_tables(tag, maxdim, res, h)


def shape_of(x):
    """Keys, nesting and value types of a harness result, without its numbers."""
    if isinstance(x, dict):
        return {k: shape_of(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [type(x).__name__] + [shape_of(v) for v in x]
    if isinstance(x, np.ndarray):
        return ("ndarray", x.shape, str(x.dtype))
    return type(x).__name__


@pytest.mark.parametrize("tag, irreps", [("g2", "all"), ("g1", "reference")])
def test_native_result_has_the_python_harness_shape(dev, tag, irreps):
    from lgn.models.autotest import lgn_tests, lgn_tests_native
    enc, dec, loader, _, _ = modules(tag, dev)
    kw = dict(unit="TeV", alpha_max=1.0, theta_max=1.0, **({"irreps": "all"} if irreps == "all" else {}))
    want, got = lgn_tests(None, enc, dec, loader, **kw), lgn_tests_native(None, enc, dec, loader, **kw)
    assert list(got) == list(want)
    assert shape_of(got) == shape_of(want)
    assert np.array_equal(got["thetas"], want["thetas"]) and got["gammas"] == want["gammas"]
    assert type(got["boost_dev_output"][0][(0, 0)]) is float and type(got["perm_invariance_dev_output"][(1, 1)]) is float
