"""Host-side checks of the whole step's loss options (ABI 18): the lgn_net_desc fields, check_desc's refusals at plan time, and
the get_real method names of NativeTrainStep.  No GPU needed."""
import ctypes as C

import pytest

from lgn import _native as N
from lgn.step import GET_REAL_CODES, get_real_code


def _desc(**kw):
    d = N.NetDesc()
    d.B, d.N, d.n_levels = 4, 12, 3
    for l, (ce, cd) in enumerate(zip((3, 3, 4, 4), (4, 4, 3, 3))):
        d.enc_channels[l], d.dec_channels[l] = ce, cd
    d.tau_s, d.tau_v, d.mlp_hidden_mul, d.mlp_nlin = 1, 8, 6, 7
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _slots(d):
    return N.lib().lgn_step_param_slots(C.byref(d), 1)


def test_abi_18_descriptor_carries_the_loss_options():
    assert N.ABI_VERSION == 19 and N.lib().lgn_abi_version() == 19
    d = N.NetDesc()
    assert d.get_real == 0 and d.jet_loss_scale == 0.0        # zero-initialised: the 'sum' step without the jet term
    assert _slots(_desc()) > 0


@pytest.mark.parametrize("code", [0, 1, 2, 3, 4])
def test_every_get_real_code_is_accepted(code):
    assert _slots(_desc(get_real=code, jet_loss_scale=0.25)) > 0


@pytest.mark.parametrize("kw,msg", [(dict(get_real=5), "get_real"), (dict(get_real=-1), "get_real"),
                                    (dict(jet_loss_scale=-1e-3), "jet_loss_scale"), (dict(dec_N=-1), "dec_N"),
                                    (dict(dec_N=4000), "dec_N")])
def test_check_desc_refuses_bad_loss_options_and_dec_N(kw, msg):
    assert _slots(_desc(**kw)) == -1
    assert msg in N.last_error()


def test_dec_N_that_fits_is_accepted():
    assert _slots(_desc(N=13, dec_N=12)) > 0


def test_get_real_names_match_the_header_codes_case_insensitively(caplog):
    assert GET_REAL_CODES == {"sum": 0, "real": 1, "imag": 2, "mean": 3, "norm": 4}
    assert get_real_code("NoRm") == 4 and get_real_code("SUM") == 0
    with caplog.at_level("WARNING"):
        assert get_real_code("abs") == 1
    assert any("abs" in r.getMessage() for r in caplog.records)
