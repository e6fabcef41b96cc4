"""Writes tests/golden/g27_emd_opts_grad.npz: inputs, values and gradients of the EMD under energyflow's options
(csrc/emd_grad_opts.hip), in the layout of g26.

This is the project's own script: it needs numpy, scipy and CPU torch (autograd for the frame's chain rule) and imports nothing from
the reference.  The expected gradients come from tests/_emd_opts_grad_ref.py (LP sensitivity on scipy's HiGHS solution of the option LP
of tests/_emd_pairs_ref.py), and every case carries its own `fd_err`: the largest difference between those gradients and central
differences of the LP's value over all its pairs -- how well the oracle itself is known.

    python tests/golden/gen_golden_g27.py

  gen_<tag>_<opt>_ev0 [B][n][3], _ev1 [B][m][3], _emd [B], _g0 [B][n][3], _g1 [B][m][3], _fd_err     events of (pT, y, phi), h = 1e-6
  rel_<tag>_<opt>_recons, _target [B][N][4], _emd [B], _g_recons, _g_target [B][N][4], _fd_err        Cartesian jets, h = 1e-5, over
                                                                                                     the particles with pT > 0
The options of a case are _emd_opts_grad_ref.case_options(tag, opt) (generic) and OPTIONS[opt] (relative).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _emd_grad_ref as G  # noqa: E402
import _emd_opts_grad_ref as GO  # noqa: E402


def main():
    out = {}
    for tag, opt in GO.GENERIC:
        a, b, o = GO.generic_case(tag, opt)
        res = [GO.emd_grad(a[i], b[i], **o) for i in range(len(a))]
        fd = [GO.fd_events(a[i], b[i], **o) for i in range(len(a))]
        pre = f"gen_{tag}_{opt}_"
        out[pre + "ev0"], out[pre + "ev1"] = a, b
        out[pre + "emd"] = np.array([r[0] for r in res])
        out[pre + "g0"], out[pre + "g1"] = np.stack([r[1] for r in res]), np.stack([r[2] for r in res])
        out[pre + "fd_err"] = np.float64(max(max(np.abs(r[1] - f[0]).max(), np.abs(r[2] - f[1]).max()) for r, f in zip(res, fd)))
    for tag, opt in GO.REL:
        r, t = G.rel_case(tag)
        o = GO.OPTIONS[opt]
        val, gr, gt = GO.emd_relative_grad(r, t, **o)
        err = 0.0
        for i in range(len(r)):
            fr, ft, mask = GO.fd_relative(r[i], t[i], **o)
            err = max(err, np.abs(gr[i] - fr)[mask[0]].max(), np.abs(gt[i] - ft)[mask[1]].max())
        pre = f"rel_{tag}_{opt}_"
        out[pre + "recons"], out[pre + "target"], out[pre + "emd"] = r, t, val
        out[pre + "g_recons"], out[pre + "g_target"], out[pre + "fd_err"] = gr, gt, np.float64(err)
    np.savez(os.path.join(HERE, "g27_emd_opts_grad.npz"), **out)
    for k, v in out.items():
        if k.endswith("_fd_err") or k.endswith("_emd"):
            print(k, v)


if __name__ == "__main__":
    main()
