"""Host-side checks of the split form of the whole-step calls on table-driven (maxdim 3) networks -- jet_features gives the encoder one
node more than the decoder reconstructs (lgn_net_desc.dec_N), data['scalars'] more input scalars per node (n_in_scalars): the
workspace queries, every refusal that must come before the first launch (placeholder pointers: a call that got as far as a launch
would fault), and the ``table_split`` keyword of the step classes on CPU modules.  No GPU needed."""
import ctypes as C

import pytest
import torch

from lgn import _native as N

CH = ((2, 3, 4), (4, 3, 2))
B, NP = 3, 12


def _desc(jet=True, K=1, maxdim=3, n=NP, **kw):
    """(descriptor of the split step on CPU models, what it points into).  K: the constructor's tau_input_scalars."""
    import __graft_entry__ as G
    from lgn.step import _step_desc
    enc, dec = G._models(n, CH[0], CH[1], torch.device("cpu"), maxdim=maxdim, jet_features=jet, tau_input_scalars=K)
    d, keep = _step_desc(enc, dec, B, True, "sum", 0.0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d, (enc, dec, keep)


def _train(d, in_scalars=8, workspace_doubles=1 << 40):
    """lgn_step_fwd_bwd_f64 with placeholder device pointers: every call here must be refused before a launch."""
    off = (C.c_int64 * 64)()
    p = 8
    return N.lib().lgn_step_fwd_bwd_f64(C.byref(d), p, p, 1000, off, off, p, p, p, in_scalars, p, workspace_doubles, p, p, None, None,
                                        None, None)


def _eval(d, in_scalars=8, workspace_doubles=1 << 40):
    off = (C.c_int64 * 64)()
    p = 8
    return N.lib().lgn_step_eval_f64(C.byref(d), p, off, off, p, p, p, in_scalars, p, workspace_doubles, p, None, None, p, p, None, None,
                                     None, None)


CALLS = {"train": _train, "eval": _eval}


def test_the_descriptor_is_the_split_table_driven_one():
    d, _keep = _desc()
    assert d.N == NP + 1 and d.dec_N == NP and d.n_in_scalars == 2 and bool(d.enc_tables[0]) and bool(d.dec_tables[0])
    assert N.lib().lgn_abi_version() == 19
    d, _keep = _desc(jet=False, K=3)
    assert d.N == NP and d.dec_N == NP and d.n_in_scalars == 3


@pytest.mark.parametrize("jet,K", [(True, 1), (True, 3), (False, 3), (False, 8)])
def test_workspace_queries_take_a_split_table_driven_descriptor(jet, K):
    d, _keep = _desc(jet=jet, K=K)
    step, ev = N.lib().lgn_step_workspace_doubles(C.byref(d)), N.lib().lgn_eval_workspace_doubles(C.byref(d))
    assert 0 < ev < step, (ev, step, N.last_error())


def test_each_network_is_carved_on_its_own_node_count():
    """The split step's workspace lies between those of the one-node-count steps on the decoder's and on the encoder's nodes: the
    decoder's buffers do not grow with the encoder's jet node."""
    lib = N.lib()
    sizes = []
    for n, jet in ((NP, False), (NP, True), (NP + 1, False)):
        d, _keep = _desc(jet=jet, n=n)
        if not jet:
            d.dec_N = 0
        sizes.append(lib.lgn_step_workspace_doubles(C.byref(d)))
    assert 0 < sizes[0] < sizes[1] < sizes[2], sizes


@pytest.mark.parametrize("call", list(CALLS))
def test_refuses_missing_input_scalars(call):
    d, _keep = _desc()
    assert CALLS[call](d, in_scalars=None) != 0
    assert "in_scalars is NULL" in N.last_error() and "2 input scalars" in N.last_error()


@pytest.mark.parametrize("call", list(CALLS))
def test_refuses_more_than_eight_input_scalars(call):
    d, _keep = _desc(n_in_scalars=9)
    assert CALLS[call](d) != 0
    assert "n_in_scalars=9" in N.last_error()
    assert N.lib().lgn_step_workspace_doubles(C.byref(d)) == -1 and N.lib().lgn_eval_workspace_doubles(C.byref(d)) == -1


@pytest.mark.parametrize("call", list(CALLS))
def test_refuses_decoder_end_stages_beyond_the_lds(call):
    d, _keep = _desc(dec_N=4000)
    assert CALLS[call](d) != 0
    assert "dec_N=4000" in N.last_error() and "LDS" in N.last_error()


@pytest.mark.parametrize("call", list(CALLS))
def test_refuses_a_latent_mismatch(call):
    d, _keep = _desc(tau_v_in=5)
    assert CALLS[call](d) != 0
    assert "pooled latent" in N.last_error()
    assert N.lib().lgn_step_workspace_doubles(C.byref(d)) == -1


@pytest.mark.parametrize("call", list(CALLS))
def test_refuses_a_short_workspace(call):
    d, _keep = _desc()
    query = N.lib().lgn_step_workspace_doubles if call == "train" else N.lib().lgn_eval_workspace_doubles
    need = query(C.byref(d))
    assert need > 0
    assert CALLS[call](d, workspace_doubles=need - 1) != 0
    assert "workspace" in N.last_error() and str(need) in N.last_error()


def test_the_step_classes_plan_the_split_form_with_the_keyword():
    """On CPU modules planning ends at the device requirement -- for a table-driven pair with table_split as for a maxdim-2 pair,
    both behind every NotImplementedError; without the keyword the refusal of the table-driven pair stands."""
    import __graft_entry__ as G
    from lgn.step import NativeEvalStep, NativeTrainStep
    cpu = torch.device("cpu")
    for cls in (NativeTrainStep, NativeEvalStep):
        for kw in (dict(jet_features=True), dict(tau_input_scalars=3), dict(jet_features=True, tau_input_scalars=7)):
            enc, dec = G._models(NP, CH[0], CH[1], cpu, maxdim=2, **kw)
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                cls(enc, dec, batch_size=B)
            enc, dec = G._models(NP, CH[0], CH[1], cpu, maxdim=3, **kw)
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                cls(enc, dec, batch_size=B, table_split=True)
            with pytest.raises(NotImplementedError, match="jet_features"):
                cls(enc, dec, batch_size=B)
            with pytest.raises(NotImplementedError, match="jet_features"):
                cls(enc, dec, batch_size=B, table_split=False)


def test_more_than_eight_input_scalars_are_refused_by_their_count():
    import __graft_entry__ as G
    from lgn.step import NativeEvalStep, NativeTrainStep
    enc, dec = G._models(NP, CH[0], CH[1], torch.device("cpu"), maxdim=3, jet_features=True, tau_input_scalars=8)
    assert enc.tau_input_scalars == 9
    for cls in (NativeTrainStep, NativeEvalStep):
        with pytest.raises(NotImplementedError, match="K = 9") as e:
            cls(enc, dec, batch_size=B, table_split=True)
        assert "maxdim 3" not in str(e.value)


def test_the_keyword_leaves_other_pairs_alone():
    """table_split changes nothing for a pair that is not split: mixed kinds are still refused by their own message."""
    import __graft_entry__ as G
    from lgn.step import NativeTrainStep
    enc, _ = G._models(NP, CH[0], CH[1], torch.device("cpu"), maxdim=3, jet_features=True)
    _, dec = G._models(NP, CH[0], CH[1], torch.device("cpu"), maxdim=2)
    with pytest.raises(NotImplementedError, match="same kind"):
        NativeTrainStep(enc, dec, batch_size=B, table_split=True)
