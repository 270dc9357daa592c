"""Host side of the JubJub / EdDSA-Poseidon entry points (no GPU): the curve constants the library derives (fk_jubjub_params) against the
oracle's JubJubBN256 and committed data, the Blake2s nonce (fk_eddsa_hash_r) against hashlib, and the exported symbols."""
import ctypes as C
import hashlib
import json
import os
import random

import numpy as np
import pytest

import bn254_ref as ref
import fawkes_circuit as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, FS = ref.R, fc.FS
SYMBOLS = ['fk_jubjub_params', 'fk_jubjub_mul_batch', 'fk_jubjub_decompress_batch', 'fk_eddsa_hash_r', 'fk_eddsa_sign_batch',
           'fk_eddsa_verify_batch', 'fk_eddsa_verify_batch_dev']


def test_params_match_oracle_and_committed_data():
    import fawkes_crypto_amd as fk
    jj = fc.JubJubBN256()
    p = fk.jubjub_params()
    assert p['d'] == jj.d and p['g'] == jj.g and p['fs'] == FS == fk.FS_MODULUS
    g = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'eddsa_golden.json')))
    assert ['%064x' % c for c in p['g']] == g['jubjub_g']
    # any of the three pointers may be NULL
    lib = fk.load_library()
    fs = np.zeros(4, np.uint64)
    assert lib.fk_jubjub_params(None, None, C.c_void_p(fs.ctypes.data)) == 0
    assert int.from_bytes(fs.tobytes(), 'little') == FS


def _hash_r_ref(sk, m):
    dig = hashlib.blake2s(sk.to_bytes(32, 'little') + m.to_bytes(32, 'little'), digest_size=32, person=b'__fawkes').digest()
    return int.from_bytes(dig, 'little') % FS


def test_hash_r_matches_hashlib():
    import fawkes_crypto_amd as fk
    from fawkes_crypto_amd import api
    rnd = random.Random(20260)
    for sk in (0, 1, FS - 1, rnd.randrange(FS)):
        for m in (0, 1, R - 1, rnd.randrange(R)):
            assert fk.eddsa_hash_r(sk, m) == _hash_r_ref(sk, m), (sk, m)
    # limbs in, limbs out: sk canonical, m Montgomery
    sk, m = rnd.randrange(FS), rnd.randrange(R)
    out = fk.eddsa_hash_r(api.int_to_limbs(sk), api._fr_rows([m]))
    assert out.dtype == np.uint64 and api.limbs_to_int(out) == _hash_r_ref(sk, m)
    # an m image equal to r is refused
    lib = fk.load_library()
    ka, bad, rho = api.int_to_limbs(1), api.int_to_limbs(R), np.zeros(4, np.uint64)
    assert lib.fk_eddsa_hash_r(api._vp(ka), api._vp(bad), api._vp(rho)) == 1
    assert b'modulus' in lib.fk_last_error(None)


def test_symbols_exported_and_listed():
    import fawkes_crypto_amd as fk
    lib = fk.load_library()
    for s in SYMBOLS:
        assert s in fk.EXPORTED_SYMBOLS, s
        assert hasattr(lib, s), s
