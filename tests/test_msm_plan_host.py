"""The window plan of a multiplication (csrc/msm.hip: make_plan, through fk_msm_plan -- host code, no GPU): the invariants the sort,
accumulate and reduce kernels rely on, swept over n around every 2^k and 1.5 * 2^k (where make_plan's rounded log2 switches), every
window-bits request 0..30 and both forms.  Invariants only: make_plan is not restated here."""
import pytest

from fawkes_crypto_amd import api

NS = sorted({1, 2} | {m + d for k in range(1, 31) for m in (1 << k, 3 << (k - 1)) for d in (-1, 0, 1)})


def _ceil_div(a, b):
    return (a + b - 1) // b


def test_fk_msm_plan_rejects_a_null_struct():
    assert api.load_library().fk_msm_plan(api.C.c_size_t(5), api.C.c_uint(0), api.C.c_int(0), None) == 1        # FK_ERR_BAD_ARG


def test_the_sweep_reaches_both_sides_of_every_rounding_step():
    assert NS[0] == 1 and NS[-1] == (3 << 29) + 1 and all(a < b for a, b in zip(NS, NS[1:]))
    for k in range(1, 31):
        assert {(1 << k) - 1, 1 << k, (1 << k) + 1, (3 << (k - 1)) - 1, 3 << (k - 1), (3 << (k - 1)) + 1} <= set(NS)


@pytest.mark.parametrize('merged', [0, 1])
def test_plan_invariants(merged):
    limits = None
    for wb in range(31):
        prev_c = 0
        for n in NS:
            p = api.msm_plan(n, wb, bool(merged))
            where = (n, wb, merged, p)
            lim = {k: p[k] for k in ('s1_tile', 's2_tile', 's2_max_hi', 'over_max', 'seg_min', 'seg_max', 'size_bins')}
            limits = limits or lim
            assert lim == limits and all(v > 0 for v in lim.values()), where          # compile-time: the same in every answer
            assert p['n'] == n, where
            W, B, c, cb, wide = p['W'], p['B'], p['c'], p['cb'], p['wide']
            # windows: the first `wide` have cb + 1 bits, the others cb; 255 bits in all
            assert cb * W + wide == 255 and 1 <= wide <= W, where
            assert c == cb + 1 and B == 1 << (c - 1) and 2 <= c <= 22, where
            # bins of the two sort passes
            assert p['nhi'] * p['nlo'] == B and p['nhi'] <= p['s2_max_hi'] and p['nlo'] <= 4096 and p['nlo'] == 1 << p['LB'], where
            # bucket reduction
            assert p['L'] * p['T'] == B and 1 <= p['L'] <= 64 and p['nblk'] == _ceil_div(p['T'], 256), where
            # first pass: chunks
            assert p['chunk'] >= 16384 and p['nchunks'] == _ceil_div(n, p['chunk']) and p['nchunks'] <= 256, where
            assert p['cap'] >= 1, where
            # the host's bound on the second pass's tiles (its grid) fits a 32-bit grid dimension
            assert W * _ceil_div(n, p['s2_tile']) + W * p['nhi'] + 1 < 1 << 32, where
            # the bound on the segment tasks leaves room beyond one task per tabled oversized bucket
            assert max(2048, W * n // p['seg_max']) + p['over_max'] + 64 > p['over_max'], where
            if wb == 0:
                assert c >= prev_c, where          # the library's own choice of c never shrinks as n grows
                prev_c = c
