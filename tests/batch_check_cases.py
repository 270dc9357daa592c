"""Cases shared by tests/test_batch_check_host.py and tests/test_gpu_batch_check.py (the batch prover's R1CS check,
include/fawkes_hip_batch_check.h): witnesses of one small system with chosen gates violated, and witnesses that are out of range or carry
a wrong ONE.  What is bad is the oracle's to say (check_cases.Want), proof by proof."""
import numpy as np

import bn254_ref as ref
import fixtures as fx
import fawkes_crypto_amd as fk
from fawkes_crypto_amd import batch as B
from helpers import r1cs_product
import check_cases as cc
from batch_cases import tile_rows

R = ref.R
GATES = (1, 63, 64, 65, 257)            # below, at and above a wave and a bitmap word; above a block
LAYOUTS = (B.Z_ROWS, B.Z_TILED)


_VARIANTS = {}


def variants(gates):
    """(instance, its R1cs, [(witness, Want)]): satisfied, one witness per set of check_cases.bad_sets, every gate bad -- made once"""
    if gates not in _VARIANTS:
        csr, z = cc.explicit_case(gates)
        zs = [z] + [cc.violate(csr, z, bad, seed=gates + k) for k, bad in enumerate(cc.bad_sets(gates))] + [cc.all_bad(csr, z)]
        wants = [cc.Want(csr, x) for x in zs]
        assert wants[0].n_bad == 0 and wants[-1].n_bad == gates
        for bad, w in zip(cc.bad_sets(gates), wants[1:]):
            assert set(bad) <= set(w.bad)
        _VARIANTS[gates] = (csr, r1cs_product(csr), list(zip(zs, wants)))
    return _VARIANTS[gates]


def laid_out(zs, layout, num_input):
    return np.ascontiguousarray(np.concatenate(zs)) if layout == B.Z_ROWS else tile_rows(zs, num_input)


# ---------------------------------------------------------------- range and ONE
def not_judged(gates, n_range, first_range, one_ok=1):
    """the whole report of a proof with an element not below r"""
    return dict(gates=gates, n_bad=0, first_bad=cc.NONE, first_abc=[[0] * 4] * 3, n_groups=0, n_bad_groups=0, n_range=n_range, first_range=first_range,
                one_ok=one_ok, gates_valid=0)


def range_cases(csr, z):
    """(name, layout) -> (three witnesses, what each report must say: None = exactly the oracle's Want of that witness, else the whole
    report).  Proof 0 is violated at gate 0, so the neighbour of an unjudged proof has something to say."""
    nv, G = len(z), csr.num_gates
    bad0 = cc.violate(csr, z, [0], seed=5)
    cases = {}
    for layout in LAYOUTS:
        zr = z.copy(); zr[1] = fk.api.int_to_limbs(R)
        cases['r at variable 1 of proof 1', layout] = ([bad0, zr, z], [None, not_judged(G, 1, 1), None])
        zm = z.copy(); zm[nv - 1] = fk.api.int_to_limbs((1 << 256) - 1); zm[nv // 2] = fk.api.int_to_limbs(R + 5)
        cases['2^256 - 1 at the last aux of proof 2', layout] = ([bad0, z, zm], [None, None, not_judged(G, 2, nv // 2)])
        zq = z.copy(); zq[nv - 1] = fk.api.int_to_limbs(R - 1)          # r - 1 is in range: judged
        cases['r - 1 is in range', layout] = ([bad0, zq, z], [None, None, None])
    z0 = [x.copy() for x in (bad0, z, z)]
    z0[1][0] = 0
    cases['a wrong ONE in one row', B.Z_ROWS] = (z0, [None, None, None])          # Want reads one_ok off the witness: only report 1
    zt = [x.copy() for x in (bad0, z, z)]
    for x in zt:
        x[0] = fx.mont_fr(2)
    cases['a wrong shared ONE', B.Z_TILED] = (zt, [None, None, None])              # every Want says one_ok = 0
    zo = [x.copy() for x in (bad0, z, z)]
    for x in zo:
        x[0] = fk.api.int_to_limbs(R)
    cases['a shared ONE that is not below r', B.Z_TILED] = (zo, [not_judged(G, 1, 0, one_ok=0)] * 3)
    return cases


def range_system():
    csr, z = cc.explicit_case(65)
    return csr, r1cs_product(csr), z
