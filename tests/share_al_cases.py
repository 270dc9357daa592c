"""Systems, witnesses and keys of tests/test_gpu_share_al_sort.py (A adopts L's bucket sort: csrc/msm.hip, key_a_pad), shared by the test and
its child process so that both build the same thing from the same seeds.

A system here has a handful of gates with LONG linear combinations: gate g's A side holds every aux variable j of the wanted density
with j % GATES == g, so the A query is exactly that density while the domain stays tiny (the transforms and H cost nothing and the
oracle's key is made in a second or two).  The B side takes a few hundred variables.  A witness need not satisfy the system: any
assignment has a well-defined proof, and the oracle proves the same assignment."""
import numpy as np

import c_oracle as co
import fixtures as fx

NUM_INPUT, GATES = 3, 4
ENV = {'FK_PROVE_SORTS_FIRST': '1', 'FK_MSM_PRE_MIN_LOG2': '8'}      # the schedule and the fixed-base levels of the benchmark size, at a small one
DENSITIES = ('all', 'none', 'alternating', 'gap', 'last')
WITNESSES = ('random', 'ones', 'zeros')


def sizes():
    """n_l just below, at and just above a whole number of first-pass and of second-pass tiles of the sort (fk_msm_plan), a few tens of thousands"""
    import fawkes_crypto_amd as fk
    p = fk.api.msm_plan(3 * 8192, 0, True)
    out = []
    for t in sorted({p['s1_tile'], p['s2_tile']}):
        out += [3 * t - 1, 3 * t, 3 * t + 1]
    return sorted(set(out)), max(p['s1_tile'], p['s2_tile'])


def rand_fr(rng, n):
    """(n, 4) uint64 below r: any such limbs are the Montgomery form of SOME element, which is all these tests need"""
    v = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    v[:, 3] = rng.integers(1, 0x3000000000000000, size=n, dtype=np.uint64)
    return v


def density(name, n, tile):
    d = np.zeros(n, np.uint8)
    if name == 'all':
        d[:] = 1
    elif name == 'alternating':
        d[0::2] = 1
    elif name == 'alternating_odd':      # as many variables as 'alternating' when n is even, one fewer when odd: see second_density
        d[1::2] = 1
    elif name == 'gap':                  # an absent run that straddles a tile boundary
        d[:] = 1
        d[tile - 100:tile + 100] = 0
    elif name == 'last':
        d[n - 1] = 1
    else:
        assert name == 'none'
    return d


def second_density(n, tile):
    """another A query with exactly as many variables as 'alternating' (the key fits both): the same pattern shifted by one, and for an odd
    n the first variable as well"""
    d = density('alternating_odd', n, tile)
    if n % 2:
        d[0] = 1
    assert d.sum() == density('alternating', n, tile).sum()
    return d


def system(n_aux, dens, seed):
    """c_oracle.R1csC whose A query takes exactly the aux variables dens marks"""
    rng = np.random.default_rng(seed)
    present = np.flatnonzero(dens).astype(np.int64)
    a_cols, b_cols = [], []
    for g in range(GATES):
        a_cols.append(np.concatenate([[0], NUM_INPUT + present[present % GATES == g]]))
        b_cols.append(np.concatenate([[g % NUM_INPUT], NUM_INPUT + np.sort(rng.choice(n_aux, size=min(150, n_aux), replace=False))]))
    c_cols = [np.array([0]) for _ in range(GATES)]

    def csr(cols):
        ptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.uint64)
        col = np.concatenate(cols).astype(np.uint32)
        return co.Csr(ptr, col, rand_fr(rng, len(col)))
    return co.R1csC(NUM_INPUT, n_aux, csr(a_cols), csr(b_cols), csr(c_cols))


def witness(name, n_aux, seed):
    rng = np.random.default_rng(seed)
    one = fx.mont_fr(1)
    z = rand_fr(rng, NUM_INPUT + n_aux)
    if name == 'ones':           # every aux scalar 1: one giant bucket, A goes through L's oversized-bucket tables
        z[NUM_INPUT:] = one
    elif name == 'zeros':
        z[:] = 0
    else:
        assert name == 'random'
    z[0] = one
    return np.ascontiguousarray(z)


def key_arrays(key):
    return dict(m=key.m, num_input=key.num_input, num_aux=key.num_aux, alpha_g1=key.alpha_g1, beta_g1=key.beta_g1, beta_g2=key.beta_g2,
                delta_g1=key.delta_g1, delta_g2=key.delta_g2, gamma_g2=key.gamma_g2,
                h=np.array(key.h), l=np.array(key.l), a=np.array(key.a), b_g1=np.array(key.b_g1), b_g2=np.array(key.b_g2))


def with_repeats_and_infinities(arrays):
    """the same key with repeated points and points at infinity of its own among A's bases (inputs and aux part)"""
    out = dict(arrays)
    a = arrays['a'].copy()
    v = NUM_INPUT
    a[v + 5] = a[v + 3]; a[v + 7] = a[v + 3]; a[v + 4] = a[2]
    a[v + 10] = 0; a[-1] = 0; a[1] = 0
    out['a'] = a
    return out


def oracle_key(arrays):
    vk = {k: arrays[k] for k in ('alpha_g1', 'beta_g1', 'beta_g2', 'gamma_g2', 'delta_g1', 'delta_g2')}
    return co.ArrayKey(arrays['m'], arrays['num_input'], arrays['num_aux'], vk, arrays['h'], arrays['l'], arrays['a'], arrays['b_g1'], arrays['b_g2'])


def case_list():
    """[(n_l, density, witness, key variant)]: every density with the dense random witness, every witness (and the key with repeated and
    infinite bases) with the alternating density -- at every size"""
    ns, tile = sizes()
    out = []
    for n in ns:
        out += [(n, d, 'random', 'plain') for d in DENSITIES]
        out += [(n, 'alternating', w, 'plain') for w in WITNESSES if w != 'random']
        out += [(n, 'alternating', 'random', 'repeats')]
    return out, tile


def case_id(c):
    return '%d-%s-%s-%s' % c


R_S = (0xA11CE, 0xB0B)
