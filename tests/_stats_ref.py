"""Plain numpy / scipy restatement of the statistics the native code of csrc/stats.hip replaces: get_stats and find_fwhm of the
reference's utils/jet_analysis/utils.py, pixelate / the average and first-n jet images of jet_images.py, and the frame of the summed
massless particles that include/lgn_amd.h specifies for modes 1 and 2 (the reference takes it from awkward / coffea).  Used by the
fixture generator (which checks it against the reference itself) and by the GPU tests."""
import numpy as np
from scipy import stats

U = 2.0 ** -52
KEYS = ("median", "IQR", "first_quartile", "third_quartile", "IDR", "MAD", "mean", "max", "min", "abs_min", "std_dev", "skew", "kurtosis",
        "FWHM", "abs_mean", "abs_mean_within_iqr", "abs_mean_within_idr")
ORDER_KEYS = ("median", "IQR", "first_quartile", "third_quartile", "IDR", "MAD", "max", "min", "abs_min")
MOMENT_KEYS = ("mean", "std_dev", "skew", "kurtosis", "abs_mean")


def find_fwhm_counts(hist, bins):
    i = np.argmax(hist)
    j = np.abs(hist - hist[i] / 2).argmin()
    return 2 * abs(bins[i] - bins[j])


def find_fwhm(err, bins):
    return find_fwhm_counts(np.histogram(err, bins=bins)[0], bins)


def none_if_nan(v):
    return None if np.isnan(v) else v


def within(res, width):
    sel = res[np.abs(res) < width]
    return np.mean(np.abs(sel)) if len(sel) else 1e32


def get_stats(res, bins):
    with np.errstate(all="ignore"):
        iqr = np.quantile(res, 0.75) - np.quantile(res, 0.25)
        idr = np.quantile(res, 0.9) - np.quantile(res, 0.1)
        return {"median": np.median(res), "IQR": iqr, "first_quartile": np.quantile(res, 0.25), "third_quartile": np.quantile(res, 0.75),
                "IDR": idr, "MAD": stats.median_abs_deviation(res), "mean": none_if_nan(np.mean(res)),
                "max": np.max(res) if len(res) else None, "min": np.min(res) if len(res) else None,
                "abs_min": np.min(np.abs(res)) if len(res) else None, "std_dev": none_if_nan(np.std(res)),
                "skew": none_if_nan(stats.skew(res)), "kurtosis": none_if_nan(stats.kurtosis(res)), "FWHM": find_fwhm(res, bins),
                "abs_mean": np.mean(np.abs(res)), "abs_mean_within_iqr": within(res, iqr), "abs_mean_within_idr": within(res, idr)}


def edges(res, alpha, num):
    med = np.median(res)
    iqr = np.quantile(res, 0.75) - np.quantile(res, 0.25)
    return np.linspace(med - alpha * iqr, med + alpha * iqr, num)


# ---- tolerances, derived from the data (never from the code under test) -----------------------------------------------------------

def quantile_neighbours(a_sorted, q):
    n = len(a_sorted)
    lo = int(np.floor((n - 1) * q))
    return a_sorted[lo], a_sorted[min(lo + 1, n - 1)]


def quantile_tolerance(a_sorted, q):
    """0 where the virtual index (n - 1) q is an integer (the quantile is a selected element: a + (b - a) 0), else
    4 * 2^-52 * max(|a_lo|, |a_hi|): three roundings plus possible contraction."""
    idx = (len(a_sorted) - 1) * q
    if idx == np.floor(idx):
        return 0.0
    lo, hi = quantile_neighbours(a_sorted, q)
    return 4 * U * max(abs(lo), abs(hi))


def order_tolerances(res):
    """|native - numpy| allowed per order statistic.  Selected elements (min, max, abs_min, the median of an odd count, a quantile at
    an integer virtual index): 0.  An interpolated value: 4 * 2^-52 * max(|a_lo|, |a_hi|) of its two neighbours.  IQR and IDR: the
    tolerances of their two quantiles plus one rounding of the difference.  MAD: the median of the deviations |a - median| -- a
    selected deviation moves by at most the median's own tolerance, so for an odd count that is the bound (0: bitwise); for an even
    count the mean of the two middle deviations adds 4 * 2^-52 * max of those two."""
    a = np.sort(res)
    n = len(a)
    t = {name: quantile_tolerance(a, q) for name, q in (("q10", 0.1), ("first_quartile", 0.25), ("third_quartile", 0.75), ("q90", 0.9))}
    t["median"] = 0.0 if n % 2 else 4 * U * max(abs(a[n // 2 - 1]), abs(a[n // 2]))
    q = {p: np.quantile(a, p) for p in (0.1, 0.25, 0.75, 0.9)}
    t["IQR"] = t["first_quartile"] + t["third_quartile"] + U * abs(q[0.75] - q[0.25])
    t["IDR"] = t["q10"] + t["q90"] + U * abs(q[0.9] - q[0.1])
    dev = np.sort(np.abs(a - np.median(a)))
    t["MAD"] = t["median"] + (0.0 if n % 2 else 4 * U * max(dev[n // 2 - 1], dev[n // 2]))
    t["max"] = t["min"] = t["abs_min"] = 0.0
    return t


def moments_longdouble(res):
    """Two-pass moments in np.longdouble and the bounds of the issue: mean within (n + 8) 2^-52 mean|x|, m_k within (n + 8) 2^-52
    mean|x - mu|^k plus the first-order effect of the mean's tolerance, skew and kurtosis by first-order propagation."""
    x = np.asarray(res, dtype=np.longdouble)
    n = len(x)
    c = (n + 8) * U
    mu = x.sum() / n
    d = x - mu
    ad = np.abs(d)
    m = {k: (d ** k).sum() / n for k in (2, 3, 4)}
    a = {k: (ad ** k).sum() / n for k in (1, 2, 3, 4)}
    e_mu = c * np.abs(x).sum() / n
    # d m_k / d mu = -k mean (x - mu)^(k-1): bounded by k mean|x - mu|^(k-1)
    e = {k: c * a[k] + k * a[k - 1] * e_mu for k in (2, 3, 4)}
    out = {"mean": (mu, e_mu), "abs_mean": (np.abs(x).sum() / n, c * np.abs(x).sum() / n)}
    with np.errstate(all="ignore"):
        std = np.sqrt(m[2])
        # |sqrt(a) - sqrt(b)| <= |a - b| / (2 sqrt(a)) to first order and <= sqrt|a - b| always (a constant column has std = 0)
        out["std_dev"] = (std, np.fmin(e[2] / (2 * std), np.sqrt(e[2])) + 4 * U * std)
        skew = m[3] / m[2] ** 1.5
        out["skew"] = (skew, e[3] / m[2] ** 1.5 + 1.5 * abs(skew) * e[2] / m[2] + 8 * U * abs(skew))
        kurt = m[4] / m[2] ** 2
        out["kurtosis"] = (kurt - 3, e[4] / m[2] ** 2 + 2 * kurt * e[2] / m[2] + 8 * U * kurt)
    return {k: (float(v), float(t)) for k, (v, t) in out.items()}


def within_longdouble(res, width):
    """abs_mean_within_* thresholded at a given width: the value in np.longdouble and the summation bound."""
    sel = np.abs(np.asarray(res, dtype=np.longdouble)[np.abs(res) < width])
    if not len(sel):
        return 1e32, 0.0
    return float(sel.sum() / len(sel)), float((len(sel) + 8) * U * sel.sum() / len(sel))


# ---- jet images ----------------------------------------------------------------------------------------------------------------------

def pixelate(jet, npix=64, maxR=1.0):
    bins = np.linspace(-maxR, maxR, npix + 1)
    eta = np.digitize(jet[:, 1], bins) - 1
    phi = np.digitize(jet[:, 2], bins) - 1
    image = np.zeros((npix, npix))
    for e, p, pt in zip(eta, phi, jet[:, 0]):
        if 0 <= e < npix and 0 <= p < npix:
            image[p, e] += pt
    return image


def frame(jets):
    """(Pt, Eta, Phi) [B][3] of the summed massless particles, summed in particle order."""
    with np.errstate(all="ignore"):
        px = np.cumsum(jets[:, :, 0] * np.cos(jets[:, :, 2]), axis=1)[:, -1]
        py = np.cumsum(jets[:, :, 0] * np.sin(jets[:, :, 2]), axis=1)[:, -1]
        pz = np.cumsum(jets[:, :, 0] * np.sinh(jets[:, :, 1]), axis=1)[:, -1]
        pt = np.hypot(px, py)
        return np.stack((pt, np.arcsinh(pz / pt), np.arctan2(py, px)), axis=-1)


def normalize(jets, fr):
    jets = jets.copy()
    if not np.isclose(fr[:, 0], 0).all():
        with np.errstate(all="ignore"):
            jets[:, :, 0] /= fr[:, 0:1]
            jets[:, :, 1] -= fr[:, 1:2]
            jets[:, :, 2] -= fr[:, 2:3]
            jets[:, :, 2] = (jets[:, :, 2] + np.pi) % (2 * np.pi) - np.pi
    return jets


def jet_images(jets, frame_jets=None, mode=0, npix=24, maxR=0.5, first_n=0):
    if mode:
        jets = normalize(jets, frame(frame_jets if mode == 2 else jets))
    images = np.stack([pixelate(j, npix, maxR) for j in jets])
    return images[:min(first_n, len(jets))], np.mean(images, axis=0)
