"""Host side of the Poseidon entry points (no GPU): the parameter generator fk_poseidon_params_new against the oracle's restatement of
PoseidonParams::new_with_salt and against committed data, the load / get round trip and its argument checks, and the rule that the
product never imports the oracle."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import bn254_ref as ref
import fawkes_circuit as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = ref.R


@pytest.mark.parametrize('t,f,p,salt', [(3, 8, 53, ''), (4, 8, 54, ''), (2, 8, 56, ''), (5, 8, 57, ''), (8, 8, 60, ''), (3, 8, 53, 'rollup-v1')])
def test_generator_matches_oracle(t, f, p, salt):
    import fawkes_crypto_amd as fk
    got, want = fk.PoseidonParams(t, f, p, salt), fc.PoseidonParams(t, f, p, salt)
    assert (got.t, got.f, got.p) == (t, f, p)
    assert got.c == want.c           # every element, canonical integers
    assert got.m == want.m
    got.free()
    got.free()                       # idempotent


def test_generator_matches_committed_data():
    import fawkes_crypto_amd as fk
    g = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'poseidon_merkle_golden.json')))
    pp = fk.PoseidonParams(3, 8, 53)
    assert '%064x' % pp.c[0][0] == g['poseidon_c0'] and '%064x' % pp.m[0][0] == g['poseidon_m00']
    assert fk.PoseidonParams(3, 8, 53, 'x').c[0][0] != pp.c[0][0]          # the salt is part of the seed


def test_load_get_round_trip_and_argument_checks():
    import fawkes_crypto_amd as fk
    from fawkes_crypto_amd import api
    lib = fk.load_library()
    src = fk.PoseidonParams(4, 8, 54)
    c, m = src.limbs()
    again = fk.PoseidonParams.from_arrays(4, 8, 54, c, m)              # Montgomery limb arrays ...
    c2, m2 = again.limbs()
    assert np.array_equal(c, c2) and np.array_equal(m, m2)
    ints = fk.PoseidonParams.from_arrays(4, 8, 54, src.c, src.m)       # ... or canonical ints
    assert np.array_equal(ints.limbs()[0], c) and ints.m == src.m
    small = fk.PoseidonParams.from_arrays(2, 1, 1, [1, 2, 3, R - 1], [5, 6, 7, 8])
    assert small.c == [[1, 2], [3, R - 1]] and small.m == [[5, 6], [7, 8]]
    # either array pointer of fk_poseidon_params_get may be NULL
    dims = (C.c_uint32 * 3)()
    assert lib.fk_poseidon_params_get(src.handle, dims, None, None) == 0 and tuple(dims) == (4, 8, 54)

    def load(t, f, p, cl, ml):
        h = C.c_void_p()
        rc = lib.fk_poseidon_params_load(C.c_uint32(t), C.c_uint32(f), C.c_uint32(p), api._vp(cl), api._vp(ml), C.byref(h))
        if rc == 0:
            lib.fk_poseidon_free(h)
        else:
            assert not h.value
        return rc

    r_limbs = api.int_to_limbs(R)
    good_c, good_m = np.zeros((2 * 2, 4), np.uint64), np.zeros((2 * 2, 4), np.uint64)
    assert load(2, 1, 1, good_c, good_m) == 0
    for where in ('c', 'm'):                                           # a limb image equal to r: FK_ERR_FORMAT
        bc, bm = good_c.copy(), good_m.copy()
        (bc if where == 'c' else bm)[3] = r_limbs
        assert load(2, 1, 1, bc, bm) == 7, where
        assert b'modulus' in lib.fk_last_error(None)
        (bc if where == 'c' else bm)[3] = api.int_to_limbs(R - 1)      # r - 1 is the largest valid image
        assert load(2, 1, 1, bc, bm) == 0
    big = np.zeros((9 * 9 * 2, 4), np.uint64)
    assert load(1, 1, 1, big, big) == 1                                # t = 1, t = 9, f + p = 0: FK_ERR_BAD_ARG
    assert load(9, 1, 1, big, big) == 1
    assert load(3, 0, 0, big, big) == 1
    for t, f, p in ((1, 8, 53), (9, 8, 53), (3, 0, 0)):
        with pytest.raises(fk.FkError) as e:
            fk.PoseidonParams(t, f, p)
        assert e.value.code == 1


def test_product_does_not_import_the_oracle():
    pkg = os.path.join(ROOT, 'fawkes-crypto_amd')
    pat = re.compile(r'^\s*(import|from)\s+.*\b(fawkes_circuit|bn254_ref)\b', re.M)
    hits = []
    for d, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith(('.py', '.hip', '.hpp', '.h')):
                text = open(os.path.join(d, fn), errors='replace').read()
                hits += ['%s: %s' % (fn, m_.group(0).strip()) for m_ in pat.finditer(text)]
    assert not hits, hits
    api_src = open(os.path.join(pkg, 'api.py')).read()
    assert 'fk_poseidon_params_new' in api_src and 'class PoseidonParams' in api_src
