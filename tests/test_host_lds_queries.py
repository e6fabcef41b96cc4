"""Plan-time LDS queries, pinned: what lgn_encoder_end_lds_bytes, lgn_decoder_end_lds_bytes, lgn_junction_lds_bytes,
lgn_assign_loss_lds_bytes and lgn_emd_lds_bytes return for 1, 9, 30, 31, 41, 150 and 191 particles, channel counts 1 .. 8 and the latent maps 'min&max', 'mean', 'mix', 'mean&min&max' and a four-block map.  These
queries decide, before any launch, whether a model takes the whole-network kernels, and they are computed from the same size
expressions as the launchers.  tests/golden/lds_query_bytes.json holds what the library returned before the launchers went through one
launch function (csrc/lds.hpp), recorded with that library selected by LGN_AMD_LIB on this module's record(); refusals (negative
returns) are part of the record.  No GPU needed."""
import json
import os

import pytest

import _util as U
from lgn import _native as N

NS = (1, 9, 30, 31, 41, 150, 191)
CS = (1, 3, 4, 6, 8)
MAPS = ("min&max", "mean", "mix", "mean&min&max", "mean&min&max&min")
TS, TV = 1, 8              # latent multiplicities of the models the tests and the benchmark build
BAD_POOL = 7 | (3 << 4)    # seven blocks: no pooling code


def _pools():
    codes = {m: N.pool_code(m) for m in MAPS}
    assert all(c is not None for c in codes.values()), codes
    codes["bad"] = BAD_POOL
    return codes


def record():
    lib = N.lib()
    out = {"encoder_end": {}, "decoder_end": {}, "junction": {}, "assign_loss": {}, "emd": {}}
    for n in NS:
        out["emd"][str(n)] = lib.lgn_emd_lds_bytes(n)
        for c in CS:
            out["assign_loss"][f"{n},{c}"] = lib.lgn_assign_loss_lds_bytes(n, c)
            for m, code in _pools().items():
                blocks = max(1, code & 7) if m != "bad" else 1
                for k in (1, 2):            # input scalars: the mass alone, or with a jet-level feature
                    out["encoder_end"][f"{n},{c},{k},{m}"] = lib.lgn_encoder_end_lds_bytes(n, c, k, c, TS, TV, code)
                out["junction"][f"{n},{c},{m}"] = lib.lgn_junction_lds_bytes(n, c, TS, TV, code, c)
                if m != "bad":
                    out["decoder_end"][f"{n},{c},{blocks * TV}"] = lib.lgn_decoder_end_lds_bytes(n, c, blocks * TV, c)
    return out


def _golden():
    with open(os.path.join(U.GOLDEN, "lds_query_bytes.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def got():
    return record()


def test_the_record_has_sizes_and_refusals(got):
    flat = [v for q in _golden().values() for v in q.values()]
    assert any(v < 0 for v in flat) and any(v > N.LDS_LIMIT for v in flat) and any(0 < v <= N.LDS_LIMIT for v in flat)
    assert {q: sorted(v) for q, v in got.items()} == {q: sorted(v) for q, v in _golden().items()}


@pytest.mark.parametrize("query", ["encoder_end", "decoder_end", "junction", "assign_loss", "emd"])
def test_lds_queries_return_the_recorded_bytes(got, query):
    ref = _golden()[query]
    assert got[query] == ref, {k: (got[query].get(k), ref[k]) for k in ref if got[query].get(k) != ref[k]}
