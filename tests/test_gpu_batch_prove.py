"""The batch prover on the GPU (include/fawkes_hip_batch.h): every stage against the per-proof entry it batches, row by row, and the whole
call against the per-proof prover, the oracle and the committed golden proof.  Every comparison is byte equality: the proof bytes are a
function of (key, witness, r, s) only, so bucket order, window width and grouping must not show."""
import random

import numpy as np
import pytest

import bn254_ref as ref
import fawkes_circuit as fc
import fixtures as fx
import witness_trace
import fawkes_crypto_amd as fk
from fawkes_crypto_amd import batch as B
from fawkes_crypto_amd import witness as W
from batch_cases import MSM_FORCED_BITS, mont_rows, msm_scalar_rows, tile_rows
from helpers import golden, g1_bases, g2_bases, params_from_oracle_key, r1cs_product, rand_fr_mont, TOXIC

pytestmark = pytest.mark.gpu
R = ref.R
TOX = {k: fx.mont_fr(v) for k, v in TOXIC.items()}


class Dev:
    """device arrays of one test, freed together"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def alloc(self, nbytes):
        p = self.ctx.dev_alloc(max(int(nbytes), 32))
        self.ptrs.append(p)
        return p

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.alloc(arr.nbytes)
        if arr.nbytes:
            self.ctx.upload(p, arr)
        return p

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.ctx.dev_free(p)


# ---------------------------------------------------------------- multiplications over shared bases
MSM_NS, MSM_COUNTS = (1, 2, 63, 64, 65, 1025), (1, 3, 65)
NUM_INPUT = 3


def _degenerate(bases, oracle, g2):
    """a point twice, a point and its negative, and an all-zero (infinity) entry, where the list is long enough"""
    b = np.array(bases, copy=True)
    n = len(b)
    if n >= 2:
        b[1] = b[0]
    if n >= 4:
        b[3] = (oracle.g2_mul if g2 else oracle.g1_mul)(b[2], fx.mont_fr(R - 1))
    if n >= 6:
        b[5] = 0
    return b


_MSM_CASES = {}


def _msm_case(ctx, oracle, n, count, g2):
    """bases, witness rows, index list and the yardstick (the single multiplication, row by row) of one shape: computed once, shared"""
    key = (n, count, g2)
    if key not in _MSM_CASES:
        rng = np.random.default_rng(1000 * n + 10 * count + g2)
        bases = _degenerate((g2_bases if g2 else g1_bases)(n, seed=n + count), oracle, g2)
        z_vars = NUM_INPUT + n
        # the scalars are variables [NUM_INPUT, NUM_INPUT + n) (L's shape); the inputs in front are random, ONE is 1 in every row (tiled: shared)
        rows = [[1] + [int(x) for x in rng.integers(0, 2 ** 62, NUM_INPUT - 1)] + row for row in msm_scalar_rows(n, count, rng)]
        idx = rng.integers(0, z_vars, n).astype(np.uint32)          # a query: any variable, repeats, ONE and inputs included
        idx[0] = NUM_INPUT
        zs = [mont_rows(r) for r in rows]
        single = ctx.msm_g2_dev if g2 else ctx.msm_g1_dev
        want = {False: [], True: []}
        with Dev(ctx) as d:
            d_bases = d.put(bases)
            for z in zs:
                for use_idx in (False, True):
                    sc = z[idx] if use_idx else z[NUM_INPUT:]
                    want[use_idx].append(single(d_bases, d.put(sc), n).tobytes())
        _MSM_CASES[key] = (bases, zs, idx, want)
    return _MSM_CASES[key]


@pytest.mark.parametrize('g2', [0, 1])
@pytest.mark.parametrize('count', MSM_COUNTS)
@pytest.mark.parametrize('n', MSM_NS)
def test_batch_msm_equals_the_single_multiplication_row_by_row(ctx, oracle, n, count, g2):
    bases, zs, idx, want = _msm_case(ctx, oracle, n, count, g2)
    z_vars = NUM_INPUT + n
    pick = MSM_NS.index(n) + MSM_COUNTS.index(count) + g2
    with Dev(ctx) as d:
        d_bases, d_idx = d.put(bases), d.put(idx)
        d_z = {B.Z_ROWS: d.put(np.concatenate(zs)), B.Z_TILED: d.put(tile_rows(zs, NUM_INPUT))}
        k = 0
        for layout in (B.Z_ROWS, B.Z_TILED):
            for use_idx in (False, True):
                bits = (MSM_FORCED_BITS[0], MSM_FORCED_BITS[1], 0)[(pick + k) % 3]         # smallest, largest, the plan's choice: every shape meets each
                k += 1
                got = B.msm_dev(ctx, d_bases, n, g2, d_z[layout], layout, z_vars, count, d_idx=d_idx if use_idx else None,
                                var_offset=0 if use_idx else NUM_INPUT, num_input=NUM_INPUT, opts=dict(window_bits_g1=bits, window_bits_g2=bits))
                assert got.shape == (count, 128 if g2 else 64)
                for i in range(count):
                    assert got[i].tobytes() == want[use_idx][i], (n, count, g2, layout, use_idx, bits, i)


@pytest.mark.parametrize('g2', [0, 1])
def test_batch_msm_every_layout_index_and_width_on_degenerate_bases_and_the_oracle(ctx, oracle, g2):
    """n = 65, count = 3: the full cross of layout x index list x window width, and on this base list (a point twice, a point and its
    negative, infinity) the single multiplication is itself held to the oracle, which decides"""
    n, count = 65, 3
    bases, zs, idx, want = _msm_case(ctx, oracle, n, count, g2)
    assert bases[1].tobytes() == bases[0].tobytes() and not bases[5].any()
    orc = oracle.msm_g2 if g2 else oracle.msm_g1
    for use_idx in (False, True):
        for i, z in enumerate(zs):
            o = orc(bases, z[idx] if use_idx else z[NUM_INPUT:]).tobytes()
            assert o == want[use_idx][i], 'the single multiplication and the oracle disagree (row %d, index list %s)' % (i, use_idx)
    with Dev(ctx) as d:
        d_bases, d_idx = d.put(bases), d.put(idx)
        d_z = {B.Z_ROWS: d.put(np.concatenate(zs)), B.Z_TILED: d.put(tile_rows(zs, NUM_INPUT))}
        for layout in (B.Z_ROWS, B.Z_TILED):
            for use_idx in (False, True):
                for bits in (MSM_FORCED_BITS[0], 5, 7, MSM_FORCED_BITS[1], 0):
                    got = B.msm_dev(ctx, d_bases, n, g2, d_z[layout], layout, NUM_INPUT + n, count, d_idx=d_idx if use_idx else None,
                                    var_offset=0 if use_idx else NUM_INPUT, num_input=NUM_INPUT, opts=dict(window_bits_g1=bits, window_bits_g2=bits))
                    assert [g.tobytes() for g in got] == want[use_idx], (g2, layout, use_idx, bits)
        # nothing to add: infinity for every proof; a width outside the compiled limits is refused
        assert not B.msm_dev(ctx, d_bases, 0, g2, d_z[B.Z_ROWS], B.Z_ROWS, NUM_INPUT + n, count).any()
        with pytest.raises(fk.FkError) as e:
            B.msm_dev(ctx, d_bases, n, g2, d_z[B.Z_ROWS], B.Z_ROWS, NUM_INPUT + n, count, var_offset=NUM_INPUT, opts=dict(window_bits_g1=15, window_bits_g2=15))
        assert e.value.code == 1


# ---------------------------------------------------------------- quotient
@pytest.mark.parametrize('count', [1, 3])
@pytest.mark.parametrize('full', [True, False])
@pytest.mark.parametrize('log_m', [1, 2, 9, 10, 11, 13])
def test_batch_quotient_equals_the_single_quotient(ctx, oracle, log_m, full, count):
    """below, at and above one LDS tile (2^10 elements) and two passes (2^11, 2^13); rows = m and m / 2 + 1.  Both quotients run the same
    pass kernel (blockIdx.y = proof), so every row is also held to the oracle, which decides"""
    m = 1 << log_m
    rows = m if full else m // 2 + 1
    with Dev(ctx) as d:
        src = [d.alloc(count * m * 32) for _ in range(3)]
        for k, p in enumerate(src):
            ctx.gen_scalars_dev(p, count * m, 77 * log_m + 3 * k + count, 0)        # behind the rows: garbage the entry has to clear
        host = [ctx.download(p, count * m * 32, np.uint64).reshape(count, m, 4) for p in src]        # the entry uses a, b, c as scratch
        want = []
        one = [d.alloc(m * 32) for _ in range(4)]
        for i in range(count):
            for k in range(3):
                ctx.dev_copy(one[k], src[k] + i * m * 32, rows * 32)
            ctx.quotient_h_dev(one[0], one[1], one[2], rows, one[3])
            want.append(ctx.download(one[3], (m - 1) * 32).tobytes())
        d_h = d.alloc(count * m * 32)
        B.quotient_dev(ctx, src[0], src[1], src[2], rows, log_m, count, d_h)
        got = ctx.download(d_h, count * m * 32).reshape(count, m * 32)
        for i in range(count):
            assert got[i, :(m - 1) * 32].tobytes() == want[i], (log_m, rows, count, i)
            assert got[i, :(m - 1) * 32].tobytes() == oracle.quotient_h(*(h[i, :rows] for h in host)).tobytes(), (log_m, rows, count, i)


# ---------------------------------------------------------------- evaluation
def _ragged_system(seed, lens_choices, gates, nin, naux):
    """random matrices with the given row lengths (zero-length rows and ONE coefficients included); not satisfiable, the product does
    not need it"""
    rng = np.random.default_rng(seed)
    nv = nin + naux
    coeffs = mont_rows([1, R - 1, 2] + [int(x) for x in rng.integers(3, 2 ** 62, 40)])

    def mat():
        lens = rng.choice(lens_choices, size=gates)
        ptr = np.zeros(gates + 1, np.uint64)
        ptr[1:] = np.cumsum(lens)
        nnz = int(ptr[-1])
        return fx.co.Csr(ptr, rng.integers(0, nv, nnz).astype(np.uint32), np.ascontiguousarray(coeffs[rng.integers(0, len(coeffs), nnz)]))

    return fx.co.R1csC(nin, naux, mat(), mat(), mat())


@pytest.mark.parametrize('system', ['random', 'ragged'])
def test_batch_eval_equals_the_single_evaluation(ctx, system):
    if system == 'random':
        csr = fx.r1cs_to_csr(ref.random_r1cs(4, 3000, 5, 3100)[0])
    else:
        csr = _ragged_system(31, [0, 1, 1, 1, 2, 3, 4, 5, 31, 32, 33, 100, 257], 700, 3, 300)
    nin, nv = csr.num_input, csr.num_input + csr.num_aux
    dr = ctx.load_r1cs(r1cs_product(csr))
    rows = dr.info()['rows']
    m = 1 << max(rows - 1, 1).bit_length()
    count = 3
    rng = np.random.default_rng(5)
    zs = []
    for i in range(count):
        z = rand_fr_mont(rng, nv, kind='witness')
        z[0] = fx.mont_fr(1)
        zs.append(z)
    with Dev(ctx) as d:
        want = []
        one = [d.alloc(m * 32) for _ in range(3)]
        for z in zs:
            ctx.r1cs_eval_dev(dr, d.put(z), *one)
            ctx.sync()
            want.append([ctx.download(p, rows * 32).tobytes() for p in one])
        for layout, z_all in ((B.Z_ROWS, np.concatenate(zs)), (B.Z_TILED, tile_rows(zs, nin))):
            outs = [d.alloc(count * m * 32) for _ in range(3)]
            for p in outs:
                ctx.gen_scalars_dev(p, count * m, 9, 0)              # the entry writes every element, the zeros behind the rows included
            B.r1cs_eval_dev(ctx, dr, d.put(z_all), layout, count, *outs)
            for k, p in enumerate(outs):
                got = ctx.download(p, count * m * 32).reshape(count, m * 32)
                for i in range(count):
                    assert got[i, :rows * 32].tobytes() == want[i][k], (system, layout, k, i)
                    assert not got[i, rows * 32:].any(), (system, layout, k, i)
    dr.free()


# ---------------------------------------------------------------- the whole call: a small random system
@pytest.fixture(scope='module')
def small(ctx, oracle):
    cs, z_in, z_aux = ref.random_r1cs(77, 900, 3, 950)
    csr = fx.r1cs_to_csr(cs)
    key = oracle.setup(csr, **TOXIC)
    params = params_from_oracle_key(key, r1cs_product(csr))
    dk, dr = ctx.load_key(params), ctx.load_r1cs(params.r1cs)
    rnd = random.Random(12)
    auxs = [list(z_aux)]
    for k in range(3):                                   # perturbed: no longer satisfying, still 256 bytes a verifier rejects
        a = list(z_aux)
        for j in rnd.sample(range(len(a)), 5 + k):
            a[j] = rnd.randrange(R)
        auxs.append(a)
    auxs.append([1] * len(z_aux))
    zs = np.stack([fx.witness_mont(z_in, a) for a in auxs])
    rs = np.stack([fx.mont_fr(rnd.randrange(R)) for _ in auxs])
    ss = np.stack([fx.mont_fr(rnd.randrange(R)) for _ in auxs])
    want = [ctx.prove_witness(dk, dr, zs[i], rs[i], ss[i]).tobytes() for i in range(len(auxs))]
    yield dict(csr=csr, key=key, params=params, dk=dk, dr=dr, zs=zs, rs=rs, ss=ss, want=want)
    dr.free(); dk.free()


def test_batch_prove_equals_the_per_proof_prover_and_the_oracle(ctx, oracle, small):
    s = small
    assert len(set(s['want'])) == 5
    got, tm = B.prove_batch(ctx, s['dk'], s['dr'], s['zs'], s['rs'], s['ss'], want_timings=True)
    assert got.shape == (5, 256) and [g.tobytes() for g in got] == s['want']
    assert tm['total_ms'] > 0 and all(tm[k] > 0 for k in ('eval_ms', 'quotient_ms', 'msm_h_ms', 'msm_l_ms', 'msm_a_ms', 'msm_b1_ms', 'msm_b2_ms', 'assemble_ms'))
    for i in (0, 4):                                     # the satisfying witness and the all-ones one also against the oracle
        a, b, c, aa, bi, ba = oracle.synthesize(s['csr'], s['zs'][i])
        assert oracle.prove(s['key'], a, b, c, s['zs'][i], aa, bi, ba, s['rs'][i], s['ss'][i]).tobytes() == s['want'][i]
    z_in = [ref.from_mont(x, R) for x in fx.co.ints(s['zs'][0][:3])]
    assert ref.verify(fx.key_to_py(s['key']), z_in[1:], ref.proof_from_borsh(got[0].tobytes()))
    # a per-proof call right behind the batch call is undisturbed
    assert ctx.prove_witness(s['dk'], s['dr'], s['zs'][1], s['rs'][1], s['ss'][1]).tobytes() == s['want'][1]
    # the call made twice gives the same bytes
    again = B.prove_batch(ctx, s['dk'], s['dr'], s['zs'], s['rs'], s['ss'])
    assert again.tobytes() == got.tobytes()
    assert B.prove_batch(ctx, s['dk'], s['dr'], s['zs'][:0], s['rs'][:0], s['ss'][:0]).shape == (0, 256)


def test_batch_prove_groups_layouts_and_widths_give_the_same_bytes(ctx, small):
    s = small
    dk, dr = s['dk'], s['dr']
    c = dk.counts()
    # a budget between the scratch of two and of three proofs: groups of 2, 2, 1
    roomy = B.plan(c['m'], c['n_l'], c['n_a'], c['n_b'], 5, dict(scratch_budget_bytes=1 << 40))
    two = B.plan(c['m'], c['n_l'], c['n_a'], c['n_b'], 2, dict(scratch_budget_bytes=1 << 40))['scratch_bytes']
    p = B.plan(c['m'], c['n_l'], c['n_a'], c['n_b'], 5, dict(scratch_budget_bytes=two))
    assert roomy['group'] == 5 and (p['group'], p['n_groups']) == (2, 3)
    got = B.prove_batch(ctx, dk, dr, s['zs'], s['rs'], s['ss'], opts=dict(scratch_budget_bytes=two))
    assert [g.tobytes() for g in got] == s['want']
    got = B.prove_batch(ctx, dk, dr, s['zs'], s['rs'], s['ss'], opts=dict(scratch_budget_bytes=1))           # groups of one
    assert [g.tobytes() for g in got] == s['want']
    with Dev(ctx) as d:
        d_rows, d_tiled = d.put(s['zs']), d.put(tile_rows(list(s['zs']), 3))
        for opts in (None, dict(window_bits_g1=5, window_bits_g2=9), dict(window_bits_g1=13, window_bits_g2=4, scratch_budget_bytes=two)):
            for d_z, layout in ((d_rows, B.Z_ROWS), (d_tiled, B.Z_TILED)):
                got = B.prove_batch_dev(ctx, dk, dr, d_z, layout, 5, s['rs'], s['ss'], opts=opts)
                assert [g.tobytes() for g in got] == s['want'], (opts, layout)
    # the scratch is the context's: trim releases it, the next call grows it again
    ctx.trim()
    assert [g.tobytes() for g in B.prove_batch(ctx, dk, dr, s['zs'], s['rs'], s['ss'])] == s['want']


def test_batch_prove_refusals(ctx, oracle, small):
    s = small
    dk, dr, zs, rs, ss = s['dk'], s['dr'], s['zs'], s['rs'], s['ss']

    def refused(code, said, fn):
        with pytest.raises(fk.FkError) as e:
            fn()
        assert e.value.code == code and said in str(e.value), str(e.value)

    # a tiled system
    tiled = ctx.load_r1cs(s['params'].r1cs, copies=2)
    refused(1, 'tiled', lambda: B.prove_batch(ctx, dk, tiled, np.zeros((2, tiled.info()['num_vars'], 4), np.uint64), rs[:2], ss[:2]))
    tiled.free()
    # a sharded key
    shard = ctx.load_key(s['params'], 0, 2)
    refused(1, 'sharded', lambda: B.prove_batch(ctx, shard, dr, zs, rs, ss))
    shard.free()
    # a system that does not belong to the key
    cs2, _, _ = ref.random_r1cs(78, 900, 3, 951)
    dr2 = ctx.load_r1cs(r1cs_product(fx.r1cs_to_csr(cs2)))
    refused(6, 'disagree', lambda: B.prove_batch(ctx, dk, dr2, np.zeros((2, 954, 4), np.uint64), rs[:2], ss[:2]))
    dr2.free()
    # above 2^20 one proof fills the device
    big = ctx.synthetic_key(1 << 21, 3, 950, 953, 600)
    refused(1, 'fk_prove_r1cs_dev', lambda: B.prove_batch(ctx, big, dr, zs, rs, ss))
    big.free()
    # an unknown layout, a null witness pointer
    with Dev(ctx) as d:
        d_z = d.put(zs)
        refused(1, 'layout', lambda: B.prove_batch_dev(ctx, dk, dr, d_z, 2, 5, rs, ss))
        refused(1, 'null', lambda: B.prove_batch_dev(ctx, dk, dr, None, B.Z_ROWS, 5, rs, ss))
    # between submit and wait: refused, and the waiting ticket still gives its own proof
    z1 = np.ascontiguousarray(zs[1])
    ticket = ctx.prove_witness_submit(dk, dr, z1, rs[1], ss[1])
    refused(1, 'outstanding', lambda: B.prove_batch(ctx, dk, dr, zs, rs, ss))
    assert ctx.prove_witness_wait(ticket).tobytes() == s['want'][1]
    # the context is as usable as before
    assert [g.tobytes() for g in B.prove_batch(ctx, dk, dr, zs[:2], rs[:2], ss[:2])] == s['want'][:2]


# ---------------------------------------------------------------- the whole call: BASELINE configs[0]
def test_batch_prove_config0_golden_proof_and_verifier(ctx):
    """four Poseidon Merkle proofs (7362 gates, domain 2^13) of four leaves in one call; index 2 is the committed golden instance"""
    g = golden('poseidon_merkle_golden.json')
    inst = []
    for k in (101, 102, g['seed'], 104):
        rnd = random.Random(k)
        leaf, sib, path = rnd.randrange(R), [rnd.randrange(R) for _ in range(32)], [rnd.randrange(2) for _ in range(32)]
        inst.append(fc.poseidon_merkle_circuit(leaf, sib, path))
    r1cs = r1cs_product(fx.r1cs_to_csr(inst[2][0].r1cs()))
    dk, vk = ctx.setup(r1cs, **TOX)
    dr = ctx.load_r1cs(r1cs)
    assert dk.counts()['m'] == 1 << 13
    zs = np.stack([fx.witness_mont(cs.z_in, cs.z_aux) for cs, _ in inst])
    rnd = random.Random(5)
    rs = np.stack([fx.mont_fr(int(g['r'], 16)) if i == 2 else fx.mont_fr(rnd.randrange(R)) for i in range(4)])
    ss = np.stack([fx.mont_fr(int(g['s'], 16)) if i == 2 else fx.mont_fr(rnd.randrange(R)) for i in range(4)])
    got = B.prove_batch(ctx, dk, dr, zs, rs, ss)
    assert got[2].tobytes().hex() == g['proof']
    assert got[0].tobytes() == ctx.prove_witness(dk, dr, zs[0], rs[0], ss[0]).tobytes()
    roots = [root for _, root in inst]
    assert len(set(roots)) == 4 and ref.from_mont(int(fx.co.ints(zs[1][1:2])[0]), R) == roots[1]
    inputs = np.ascontiguousarray(zs[:, 1:2])                          # every proof's own root
    assert fk.verify_batch(ctx, fk.vk_to_borsh(vk), inputs, got).all()
    assert not fk.verify_batch(ctx, fk.vk_to_borsh(vk), inputs[::-1], got).any()
    dr.free(); dk.free()


# ---------------------------------------------------------------- from the given rows
_P3 = fc.PoseidonParams(3, 8, 53)


def _merkle_params(k):
    rnd = random.Random(100 + k)
    return rnd.randrange(R), [rnd.randrange(R) for _ in range(2)], [rnd.randrange(2) for _ in range(2)]


def test_prove_given_batch_equals_the_per_proof_proofs_of_the_one_instance_key(ctx):
    """the depth-2 Merkle gadget, traced once; three given rows -> three independent proofs of the ONE-instance key"""
    with witness_trace.trace() as t:
        first = fc.poseidon_merkle_circuit(*_merkle_params(0), 2, _P3)[0]
    prog, g0 = t.program(first)
    given = [g0] + [[fc.poseidon_merkle_proof_root(leaf, sib, path, _P3), leaf, *sib, *path] for leaf, sib, path in (_merkle_params(k) for k in (1, 2))]
    zs = [fx.witness_mont(first.z_in, first.z_aux)]
    for gv in given[1:]:
        z = prog.run_host([gv])
        assert len(z) == len(first.z_in) + len(first.z_aux)
        zs.append(fk.api._fr_rows(z))
    r1cs = r1cs_product(fx.r1cs_to_csr(first.r1cs()))
    dk, _ = ctx.setup(r1cs, **TOX)
    dr = ctx.load_r1cs(r1cs)
    dp = W.load(ctx, prog)
    rs = np.stack([fx.mont_fr(0x5eed0 + i) for i in range(3)])
    ss = np.stack([fx.mont_fr(0xfeed0 + i) for i in range(3)])
    want = [ctx.prove_witness(dk, dr, zs[i], rs[i], ss[i]).tobytes() for i in range(3)]
    assert len(set(want)) == 3
    got = B.prove_given_batch(ctx, dp, dk, dr, given, rs, ss)
    assert got.shape == (3, 256) and [g.tobytes() for g in got] == want
    dp.free(); dr.free(); dk.free()
