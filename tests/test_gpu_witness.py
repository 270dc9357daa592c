"""Device witness generation (csrc/witness.hip through fawkes_crypto_amd/witness.py) against the Python-integer interpreter
`WitnessProgram.run_host` and against the witnesses the circuit builder of oracle/fawkes_circuit.py computes itself: hand-made programs
that isolate every opcode and edge of the interpreter, the traced Merkle / eddsa / transaction circuits as tiled batches, and the path
from given rows to proof bytes.  Every comparison is byte or integer equality."""
import random

import numpy as np
import pytest

import bn254_ref as ref
import fawkes_circuit as fc
import fixtures as fx
import witness_trace
import fawkes_crypto_amd as fk
from fawkes_crypto_amd import witness as W
from helpers import r1cs_product, golden, TOXIC
from test_gpu_tiled import _tile_z

pytestmark = pytest.mark.gpu
R = ref.R
TOX = {k: fx.mont_fr(v) for k, v in TOXIC.items()}
COPIES = (1, 63, 64, 65, 130)


def _special(rnd):
    return [0, 1, 2, R - 1, 1 << 253, rnd.randrange(R)]


def given_rows(n_given, copies, seed):
    """per-copy values drawn from {0, 1, 2, r - 1, 2^253, random}: column j of copy c walks the six in a stride of its own, so that two
    columns meet in every pair (zero numerators, zero denominators, both) within 36 copies"""
    rnd = random.Random(seed)
    return [[_special(rnd)[(c // 6 ** (j % 2) + j // 2 + seed) % 6] for j in range(n_given)] for c in range(copies)]


def var(v, k=1):
    return (1 + v, k)


# ---------------------------------------------------------------- hand-made programs
def prog_given():
    p = W.WitnessProgram()
    for _ in range(3):
        p.given()
    return p


def prog_mul():
    p = W.WitnessProgram()
    a, b = p.given(), p.given()
    la, lb = p.lc([var(a)]), p.lc([var(b)])
    p.mul(la, lb)
    p.mul(la, la)                                   # one combination, evaluated once
    p.mul(p.lc([var(a, 3), var(b, R - 2), (0, 7)]), p.lc([var(b), var(a)]))
    return p


def prog_div0():
    p = W.WitnessProgram()
    a, b = p.given(), p.given()
    la, lb = p.lc([var(a)]), p.lc([var(b)])
    p.div0(la, lb)                                  # the rows hold x / 0, 0 / x and 0 / 0
    p.div0(lb, la)
    p.div0(la, la)
    p.div0(p.lc([var(a), (0, 1)]), p.lc([var(a), var(b, R - 1)]))       # a - b: zero wherever the two columns agree
    return p


def prog_inv0():
    p = W.WitnessProgram()
    a = p.given()
    p.inv0(p.lc([var(a)]))
    p.inv0(p.lc([]))                                # 1 / 0 = 0
    p.inv0(p.lc([(0, 1)]))                          # 1 / 1
    p.inv0(p.lc([(0, R - 1)]))                      # 1 / (r - 1) = r - 1
    p.inv0(p.lc([var(a), var(a, R - 1)]))           # a - a
    return p


def prog_bits_run():
    p = W.WitnessProgram()
    a = p.given()
    l = p.lc([var(a)])
    for i in range(254):
        p.bit(l, i)
    return p


def prog_bits_interleaved():
    p = W.WitnessProgram()
    a, b = p.given(), p.given()
    la, lb = p.lc([var(a)]), p.lc([var(b)])
    p.bit(la, 3)
    m = p.mul(la, lb)
    p.bit(la, 200)                                  # the same combination again, not consecutive
    p.bit(lb, 253)                                  # consecutive BITs of different combinations
    p.bit(lb, 31)
    p.bit(lb, 32)
    p.given()
    p.bit(la, 0)
    p.div0(lb, p.lc([var(m), (0, 1)]))
    lm = p.lc([var(m), var(a, 2)])
    p.bit(lm, 255)                                  # always 0: every value is below 2^254
    p.bit(lm, 64)
    p.inv0(lm)
    p.bit(lm, 64)
    return p


def prog_empty_lc():
    p = W.WitnessProgram()
    a = p.given()
    e = p.lc([])
    p.mul(e, p.lc([var(a)]))
    p.div0(p.lc([var(a)]), e)
    p.bit(e, 0)
    p.public(e)
    return p


def prog_one_lc():
    """ONE alone, and no coefficient other than ONE anywhere: the descriptor's lc_val is NULL"""
    p = W.WitnessProgram()
    a, b = p.given(), p.given()
    one = p.lc([(0, 1)])
    p.mul(one, p.lc([var(a)]))
    p.mul(p.lc([var(a), var(b), (0, 1), (0, 1)]), p.lc([var(b), var(b), var(a)]))      # ONE twice, a column twice
    p.bit(one, 0)
    p.public(one)
    assert p.desc().lc_val is None
    return p


def prog_long_lc():
    """600 terms over 40 variables: longer than any group of four, unit and other coefficients mixed, ONE among them several times"""
    rnd = random.Random(600)
    p = W.WitnessProgram()
    g = [p.given() for _ in range(40)]
    terms = [(0, rnd.randrange(R)) if i % 97 == 5 else var(rnd.choice(g), 1 if i % 3 == 0 else rnd.randrange(R)) for i in range(600)]
    l = p.lc(terms)
    p.mul(l, p.lc([(0, 1)]))
    for n in (1, 2, 3, 4, 5, 7, 8, 9):              # every remainder of the groups of four, units only and products only
        p.mul(p.lc([var(g[i]) for i in range(n)]), p.lc([var(g[i], 5 + i) for i in range(n)]))
    p.public(l)
    return p


def prog_chain():
    """every operation names the variable written immediately before it"""
    p = W.WitnessProgram()
    v = p.given()
    for i in range(12):
        prev = p.lc([var(v)])
        if i % 4 == 0:
            v = p.mul(prev, p.lc([var(v), (0, i + 1)]))
        elif i % 4 == 1:
            v = p.div0(p.lc([(0, 1)]), prev)
        elif i % 4 == 2:
            v = p.inv0(prev)
        else:
            v = p.bit(prev, 0)
            v = p.mul(p.lc([var(v), var(v - 1)]), p.lc([var(v - 2)]))
    return p


def prog_four_inputs():
    p = W.WitnessProgram()
    a, b = p.given(), p.given()
    m = p.mul(p.lc([var(a)]), p.lc([var(b)]))
    p.public(p.lc([var(m)]))
    p.public(p.lc([var(a), var(b, 2), (0, 3)]))
    p.public(p.lc([var(a)]))
    assert p.num_input == 4
    return p


PROGRAMS = dict(given=prog_given, mul=prog_mul, div0=prog_div0, inv0=prog_inv0, bits_run=prog_bits_run, bits_interleaved=prog_bits_interleaved,
                empty_lc=prog_empty_lc, one_lc=prog_one_lc, long_lc=prog_long_lc, chain=prog_chain, four_inputs=prog_four_inputs)


@pytest.fixture(scope='module')
def micro(ctx):
    """name -> (program, resident program), loaded once"""
    out = {name: (p, W.load(ctx, p)) for name, p in ((n, f()) for n, f in PROGRAMS.items())}
    yield out
    for _, dp in out.values():
        dp.free()


@pytest.mark.parametrize('copies', COPIES)
@pytest.mark.parametrize('name', sorted(PROGRAMS))
def test_micro_program_equals_run_host(ctx, micro, name, copies):
    p, dp = micro[name]
    rows = given_rows(p.n_given, copies, seed=copies + len(name))
    want = fk.api._fr_rows(p.run_host(rows))
    got = W.generate(ctx, dp, rows)
    assert got.shape == want.shape == (p.witness_len(copies), 4)
    assert got.tobytes() == want.tobytes()


def test_the_rows_hold_the_zero_cases():
    rows = given_rows(2, 63, seed=0)
    assert any(a and not b for a, b in rows) and any(b and not a for a, b in rows) and any(not a and not b for a, b in rows)
    assert {0, 1, 2, R - 1, 1 << 253} <= {a for a, _ in rows}


def test_explicit_unit_coefficients_equal_null_lc_val(ctx, micro):
    p, _ = micro['one_lc']
    dp = W.load(ctx, p.desc(explicit_ones=True))
    rows = given_rows(p.n_given, 65, seed=3)
    assert W.generate(ctx, dp, rows).tobytes() == fk.api._fr_rows(p.run_host(rows)).tobytes()
    assert dp.info()['distinct_coefficients'] == 2           # ONE, and the constant 1 + 1 the loader folded
    dp.free()


def expected_info(p):
    """what fk_witness_program_info reports, derived from the program"""
    evals = len(p.input_lc)
    for v, (op, a0, a1) in enumerate(zip(p.op, p.arg0, p.arg1)):
        if op == W.BIT:
            evals += not (v and p.op[v - 1] == W.BIT and p.arg0[v - 1] == a0)
        elif op in (W.MUL, W.DIV0):
            evals += 1 if a0 == a1 else 2
        elif op == W.INV0:
            evals += 1
    return dict(num_input=p.num_input, num_aux=p.num_aux, n_given=p.n_given, lcs=len(p.lcs), lc_terms=sum(len(l) for l in p.lcs),
                distinct_coefficients=len({k for l in p.lcs for _, k in l} | {1}), lc_evaluations=evals, inversions=p.op.count(W.DIV0) + p.op.count(W.INV0))


def test_info_of_hand_made_programs(micro):
    p, dp = micro['bits_run']
    assert dp.info() == expected_info(p) and dp.info()['lc_evaluations'] == 1
    p, dp = micro['bits_interleaved']
    assert dp.info() == expected_info(p) and dp.info()['lc_evaluations'] == 1 + 2 + 1 + 1 + 1 + 2 + 1 + 1 + 1
    p, dp = micro['mul']
    assert dp.info() == expected_info(p) and dp.info()['lc_evaluations'] == 5


def test_zero_copies_write_nothing(ctx, micro):
    p, dp = micro['mul']
    pattern = np.arange(64, dtype=np.uint64)
    d_z, d_g = ctx.dev_alloc(pattern.nbytes), ctx.dev_alloc(64)
    ctx.upload(d_z, pattern)
    W.generate_dev(ctx, dp, d_g, 0, d_z)
    ctx.sync()
    assert np.array_equal(ctx.download(d_z, pattern.nbytes, np.uint64), pattern)
    assert W.generate(ctx, dp, []).shape == (0, 4)
    # past 32-bit variable indices: refused before anything is queued
    with pytest.raises(fk.FkError) as e:
        W.generate_dev(ctx, dp, d_g, 1 << 30, d_z)
    assert e.value.code == 1
    ctx.sync()
    assert np.array_equal(ctx.download(d_z, pattern.nbytes, np.uint64), pattern)
    ctx.dev_free(d_z); ctx.dev_free(d_g)


def test_load_refuses_an_invalid_program(ctx, micro):
    p = prog_mul()
    p.arg1[2] = 99
    with pytest.raises(fk.FkError) as e:
        W.load(ctx, p)
    assert e.value.code == 1 and 'variable 2' in str(e.value)
    p = prog_mul()
    d = p.desc()
    d.keep[6][0] = fk.api.int_to_limbs(R)
    with pytest.raises(fk.FkError) as e:
        W.load(ctx, d)
    assert e.value.code == 7
    # the context is as it was
    q, dq = micro['given']
    rows = given_rows(3, 2, seed=1)
    assert W.generate(ctx, dq, rows).tobytes() == fk.api._fr_rows(q.run_host(rows)).tobytes()


def test_the_wrapper_refuses_a_given_value_not_below_r(ctx, micro):
    _, dp = micro['given']
    with pytest.raises(ValueError):
        W.generate(ctx, dp, [[0, R, 1]])
    bad = np.zeros((3, 4), np.uint64)
    bad[2] = fk.api.int_to_limbs(R)
    with pytest.raises(ValueError):
        W.generate(ctx, dp, bad)
    bad[2] = fk.api.int_to_limbs(R - 1)
    assert W.generate(ctx, dp, bad).shape == (4, 4)


# ---------------------------------------------------------------- traced circuits
class Gadget:
    """Three distinct instances of one circuit.  The first is built by the circuit builder under the tracer: its program, its given row
    and its witness are the builder's.  Building a signature circuit costs seconds of host Python, so the other two are given rows
    computed natively (the same function reproduces the first instance's traced row) with `run_host`'s witness."""

    def __init__(self, params, circuit, native_given, n=3):
        with witness_trace.trace() as t:
            first = circuit(*params(0))
        self.first = first
        self.prog, g0 = t.program(first)
        self.given = [native_given(*params(k)) for k in range(n)]
        assert self.given[0] == g0
        self.z_ints = [[*first.z_in, *first.z_aux]] + [self.prog.run_host([g]) for g in self.given[1:]]
        self.zs = [fx.witness_mont(first.z_in, first.z_aux)] + [fk.api._fr_rows(z) for z in self.z_ints[1:]]
        self.num_gates = len(first.gates)
        self._r1cs = None

    @property
    def r1cs(self):
        if self._r1cs is None:
            self._r1cs = r1cs_product(fx.r1cs_to_csr(self.first.r1cs()))
        return self._r1cs


_P3, _P4, _JJ = fc.PoseidonParams(3, 8, 53), fc.PoseidonParams(4, 8, 54), fc.JubJubBN256()


def _preimage(x):
    """the cofactor preimage CEdwards.subgroup_decompress allocates (ecc.rs:69-80)"""
    return list(_JJ.mul(_JJ.subgroup_decompress(x), pow(8, -1, fc.FS)))


def _merkle_params(k):
    rnd = random.Random(100 + k)
    return rnd.randrange(R), [rnd.randrange(R) for _ in range(2)], [rnd.randrange(2) for _ in range(2)]


def _merkle_given(leaf, sibling, path):
    return [fc.poseidon_merkle_proof_root(leaf, sibling, path, _P3), leaf, *sibling, *path]


def _eddsa_params(k):
    rnd = random.Random(200 + k)
    return rnd.randrange(fc.FS), rnd.randrange(R), rnd.randrange(fc.FS)


def _eddsa_given(sk, m, rho):
    s, r_x, a_x = fc.eddsaposeidon_sign(sk, m, rho, _P4, _JJ)
    return [m, s, r_x, a_x, *_preimage(a_x), *_preimage(r_x)]


def _rollup_params(k):
    rnd = random.Random(300 + k)
    return rnd.randrange(fc.FS), 500 + k, 400 + k, [rnd.randrange(R) for _ in range(2)], [rnd.randrange(2) for _ in range(2)], rnd.randrange(fc.FS)


def _rollup_given(sk, bal_old, bal_new, sibling, path, rho):
    a_x = _JJ.mul(_JJ.g, sk)[0]
    leaf_old, leaf_new = fc.poseidon([a_x, bal_old], _P3), fc.poseidon([a_x, bal_new], _P3)
    roots = [fc.poseidon_merkle_proof_root(l, sibling, path, _P3) for l in (leaf_old, leaf_new)]
    s, r_x, _ = fc.eddsaposeidon_sign(sk, leaf_new, rho, _P4, _JJ)
    return [*roots, a_x, bal_old, bal_new, *sibling, *path, s, r_x, *_preimage(a_x), *_preimage(r_x)]


_BUILD = dict(merkle2=(_merkle_params, lambda *a: fc.poseidon_merkle_circuit(*a, 2, _P3)[0], _merkle_given),
              eddsa=(_eddsa_params, lambda *a: fc.eddsa_circuit(*a, _P4, _JJ)[0], _eddsa_given),
              rollup2=(_rollup_params, lambda *a: fc.rollup_tx_circuit(*a, 2), _rollup_given))
_GADGETS = {}


@pytest.fixture(scope='module')
def gadget(ctx):
    """name -> (Gadget, resident program), each traced and loaded on first use and shared by the tests of this module"""
    def get(name):
        if name not in _GADGETS:
            g = Gadget(*_BUILD[name])
            _GADGETS[name] = (g, W.load(ctx, g.prog))
        return _GADGETS[name]
    yield get
    for _, dp in _GADGETS.values():
        dp.free()
    _GADGETS.clear()


@pytest.mark.parametrize('name', ['merkle2', 'eddsa', 'rollup2'])
def test_traced_circuit_67_copies_equal_the_host_witnesses(ctx, gadget, name):
    g, dp = gadget(name)
    assert len({tuple(x) for x in g.given}) == 3
    picks = [k % 3 for k in range(67)]
    want = _tile_z(g.zs, g.prog.num_input, picks)
    got = W.generate(ctx, dp, [g.given[k] for k in picks])
    assert got.shape == want.shape and got.tobytes() == want.tobytes()
    info = dp.info()
    assert info == expected_info(g.prog)
    c = g.prog.counts()
    squares = sum(1 for op, a0, a1 in zip(g.prog.op, g.prog.arg0, g.prog.arg1) if op in (W.MUL, W.DIV0) and a0 == a1)
    assert info['lc_evaluations'] == c['BIT_runs'] + 2 * (c['MUL'] + c['DIV0']) - squares + c['INV0'] + g.prog.num_input - 1
    assert info['inversions'] == c['DIV0'] + c['INV0']
    if name != 'merkle2':
        assert (c['BIT'], c['BIT_runs']) == (756, 4)         # 756 bits cost 4 evaluations


def _constraints_hold(ctx, dr, z, rows):
    """a_i * b_i == c_i on the given rows of the resident system, evaluated on the device from the witness z"""
    n_rows = dr.info()['rows']
    m = 1 << max(n_rows - 1, 1).bit_length()
    d_z = ctx.dev_alloc(z.nbytes)
    outs = [ctx.dev_alloc(m * 32) for _ in range(3)]
    ctx.upload(d_z, z)
    ctx.r1cs_eval_dev(dr, d_z, *outs)
    ctx.sync()
    lo, hi = rows
    a, b, c = ([fk.api.limbs_to_int(x) for x in ctx.download(o + 32 * lo, 32 * (hi - lo), np.uint64).reshape(-1, 4)] for o in outs)
    for o in [d_z] + outs:
        ctx.dev_free(o)
    rinv = pow(1 << 256, -1, R)
    return all(x * y * rinv % R == w for x, y, w in zip(a, b, c))


@pytest.mark.parametrize('name,s_at', [('eddsa', 1), ('rollup2', 9)])
def test_a_corrupted_signature_is_generated_like_any_other(ctx, gadget, name, s_at):
    """the reference's WitnessCS behaviour: a witness that violates the circuit is no error.  Copy 5's s is off by one: the device writes
    what run_host computes for that row, the constraints of that copy fail and those of its neighbour hold.  (DeviceR1cs.check_witness
    is the length check of the prove calls; it passes -- what rejects the witness is the constraint system, evaluated here.)"""
    g, dp = gadget(name)
    assert g.prog.n_given == {'eddsa': 8, 'rollup2': 15}[name]
    copies, picks = 67, [k % 3 for k in range(67)]
    rows = [list(g.given[k]) for k in picks]
    rows[5][s_at] = (rows[5][s_at] + 1) % fc.FS
    z_bad_one = g.prog.run_host([rows[5]])
    ni, na = g.prog.num_input, g.prog.num_aux
    good = g.z_ints[picks[5]]
    assert z_bad_one[:ni] == good[:ni] and z_bad_one[ni:] != good[ni:]
    zs = list(g.zs) + [fk.api._fr_rows(z_bad_one)]
    want = _tile_z(zs, ni, picks[:5] + [3] + picks[6:])
    got = W.generate(ctx, dp, rows)
    assert got.tobytes() == want.tobytes()
    dr = ctx.load_r1cs(g.r1cs, copies=copies)
    dr.check_witness(got)
    G = g.num_gates
    assert dr.info()['rows'] == copies * G + 1 + copies * (ni - 1)
    assert _constraints_hold(ctx, dr, got, (4 * G, 5 * G))
    assert not _constraints_hold(ctx, dr, got, (5 * G, 6 * G))
    dr.free()


# ---------------------------------------------------------------- end to end
def test_prove_given_equals_prove_witness_on_the_host_witness(ctx, gadget):
    g, dp = gadget('rollup2')
    picks = [2, 0, 1]
    dk, _ = ctx.setup(g.r1cs, copies=3, **TOX)
    dr = ctx.load_r1cs(g.r1cs, copies=3)
    r, s = fx.mont_fr(0x5eed5), fx.mont_fr(0xfeed5)
    z = _tile_z(g.zs, g.prog.num_input, picks)
    want = ctx.prove_witness(dk, dr, z, r, s)
    got = W.prove_given(ctx, dk, dr, dp, [g.given[k] for k in picks], r, s)
    assert got.tobytes() == want.tobytes() and len(got.tobytes()) == 256
    with pytest.raises(fk.FkError):                 # a batch of another size than the system's
        W.prove_given(ctx, dk, dr, dp, [g.given[0]], r, s)
    dr.free(); dk.free()


def test_golden_transaction_proof_from_the_traced_program(ctx):
    """tests/golden/rollup_tx_golden.json (made by the C oracle) from the depth-32 program with copies = 1, where the tiled order is the
    plain order: given row -> device witness -> proof, the committed 256 bytes"""
    g = golden('rollup_tx_golden.json')
    rnd = random.Random(g['seed'])
    sibling, path = [rnd.randrange(R) for _ in range(32)], [rnd.randrange(2) for _ in range(32)]
    with witness_trace.trace() as t:
        cs = fc.rollup_tx_circuit(int(g['sk'], 16), g['bal_old'], g['bal_new'], sibling, path, int(g['rho'], 16))
    prog, given = t.program(cs)
    c = prog.counts()
    assert (prog.num_aux, c['GIVEN'], c['MUL'], c['DIV0'], c['INV0'], c['BIT'], c['BIT_runs']) == (19298, 75, 17852, 611, 4, 756, 4)
    assert '%064x' % cs.z_in[1] == g['old_root'] and len(cs.gates) == g['num_gates']
    dp = W.load(ctx, prog)
    assert W.generate(ctx, dp, [given]).tobytes() == fx.witness_mont(cs.z_in, cs.z_aux).tobytes()
    r1cs = r1cs_product(fx.r1cs_to_csr(cs.r1cs()))
    dk, _ = ctx.setup(r1cs, **TOX)
    dr = ctx.load_r1cs(r1cs)
    got = W.prove_given(ctx, dk, dr, dp, [given], fx.mont_fr(int(g['r'], 16)), fx.mont_fr(int(g['s'], 16)))
    assert got.tobytes().hex() == g['proof']
    dr.free(); dk.free(); dp.free()
