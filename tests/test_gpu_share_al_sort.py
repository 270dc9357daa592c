"""A adopts L's bucket sort (csrc/msm.hip: key_a_pad, msm_begin's lender; csrc/prover.hip: witness_begin): A's aux bases are kept a second
time in L's index space, with infinity where a variable takes no part in A, so that A's aux part is a multiplication over L's scalars
that reads L's sort from another lane; A's inputs are a small multiplication of their own and the two sums are added.

The proof bytes of that path are compared with the same library with FK_PROVE_SHARE_AL_SORT=0 (a child process each: the switches are
read once per process) and with the C oracle, under the sorts-first schedule with fixed-base levels (share_al_cases.ENV), and once
more with no levels at all (FK_MSM_PRECOMP=0: the W-bucket-set kernels read the adopted sort).  n_l sits just below, at and just above
a whole number of the sort's tiles; the A queries and witnesses are the ones listed in share_al_cases.case_list.

Where a and l are in different forms -- A's query so small that it gets no levels while l has them ('none', 'last' with levels on) --
the precondition sends A down its own path: the padded array is refused there, and the bytes are the same again."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import share_al_cases as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES, TILE = sc.case_list()


def _child(kdir, env):
    e = dict(os.environ)
    for k in list(e):
        if k.startswith(('FK_MSM_', 'FK_NTT_', 'FK_PROVE_', 'FK_SPMV_', 'FK_DEBUG')): del e[k]
    e.update(sc.ENV)
    e.update(env)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_share_al_child.py'), kdir], env=e, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and out.stdout.rstrip().endswith('DONE'), (env, out.stdout[-1500:], out.stderr[-3000:])
    res = {'case': {}}
    for line in out.stdout.splitlines():
        if line.startswith('RESULT '):
            j = json.loads(line[7:])
            if j['tag'] == 'case':
                res['case'][j['id']] = j
            else:
                res[j['tag']] = j
    return res


@pytest.fixture(scope='module')
def world(oracle, tmp_path_factory):
    """the oracle's keys (handed to the children as files) and its proofs of every case, computed once"""
    import fixtures as fx
    from helpers import TOXIC
    kdir = str(tmp_path_factory.mktemp('share_al_keys'))
    r, s = fx.mont_fr(sc.R_S[0]), fx.mont_fr(sc.R_S[1])
    keys, want = {}, {}

    def prove(key, csr, z):
        a, b, c, aa, bi, ba = oracle.synthesize(csr, z)
        return oracle.prove(key, a, b, c, z, aa, bi, ba, r, s, threads=8).tobytes().hex()      # (bellman's multicore split: the same bytes)

    for c in CASES:
        n, dname, wname, variant = c
        if (n, dname) not in keys:
            csr = sc.system(n, sc.density(dname, n, TILE), seed=n)
            arrays = sc.key_arrays(oracle.setup(csr, **TOXIC))
            np.savez(os.path.join(kdir, '%d-%s.npz' % (n, dname)), **arrays)
            keys[(n, dname)] = (csr, arrays)
        csr, arrays = keys[(n, dname)]
        key = sc.oracle_key(sc.with_repeats_and_infinities(arrays) if variant == 'repeats' else arrays)
        want[sc.case_id(c)] = prove(key, csr, sc.witness(wname, n, seed=n + 1))
    # the further scenarios of the child, on the middle size and the alternating query
    n = sc.sizes()[0][1]
    csr1, arrays = keys[(n, 'alternating')]
    key = sc.oracle_key(arrays)
    csr2 = sc.system(n, sc.second_density(n, TILE), seed=n + 7)
    z1, z2 = sc.witness('random', n, seed=n + 1), sc.witness('random', n, seed=n + 2)
    want['two_systems'] = [prove(key, cs, z) for cs, z in ((csr1, z1), (csr2, z1), (csr2, z2), (csr1, z2), (csr1, z1))]
    want['wit'] = [prove(key, csr1, z) for z in (z1, z2, sc.witness('ones', n, seed=0), sc.witness('zeros', n, seed=0))]
    return dict(kdir=kdir, want=want, n_mid=n)


@pytest.fixture(scope='module')
def shared(world):
    return _child(world['kdir'], {})


@pytest.fixture(scope='module')
def shared_no_levels(world):
    return _child(world['kdir'], {'FK_MSM_PRECOMP': '0'})


@pytest.fixture(scope='module')
def own_sort(world):
    return _child(world['kdir'], {'FK_PROVE_SHARE_AL_SORT': '0'})


@pytest.mark.parametrize('case', CASES, ids=sc.case_id)
def test_shared_sort_gives_the_bytes_of_the_own_sort_and_of_the_oracle(case, world, shared, shared_no_levels, own_sort):
    cid = sc.case_id(case)
    n, dname, _, _ = case
    want = world['want'][cid]
    a, b, c = shared['case'][cid], shared_no_levels['case'][cid], own_sort['case'][cid]
    assert c['proof'] == want and c['again'] == want, 'A with its own sort differs from the oracle'
    assert a['proof'] == want and a['again'] == want, 'the shared sort (levels) differs from the oracle'
    assert b['proof'] == want and b['again'] == want, 'the shared sort (no levels) differs from the oracle'
    # which path ran: the switch keeps A's own sort; without levels a and l are always in one form; with levels an A query of a
    # handful of points has none while l has them, and the precondition refuses
    assert not c['pad']['in_place'] and (c['levels']['a'] > 1) == (dname not in ('none', 'last'))
    assert (b['pad']['arrays'], b['pad']['points'], b['pad']['levels'], b['pad']['refused']) == (1, n, 0, False)
    assert a['levels']['l'] > 1
    if dname in ('none', 'last'):
        assert a['pad']['refused'] and not a['pad']['in_place'] and a['levels']['a'] == 0
    else:
        assert (a['pad']['arrays'], a['pad']['points'], a['pad']['levels'], a['pad']['refused']) == (1, n, a['levels']['l'], False)
        assert a['pad']['bytes'] == (n + 1) * 64 + (a['levels']['l'] - 1) * n * 64
        assert a['levels']['a'] > 1, 'a keeps its own levels: another context may be proving from them'


@pytest.mark.parametrize('mode', ['levels', 'no_levels', 'own_sort'])
def test_second_system_with_another_a_query_on_the_same_key(mode, world, shared, shared_no_levels, own_sort):
    """two resident systems whose A queries take different variables (equally many), proved in turn with one key in one context: the padded
    array is rebuilt whenever the query's fingerprint changes"""
    res = dict(levels=shared, no_levels=shared_no_levels, own_sort=own_sort)[mode]['two_systems']
    assert res['proofs'] == world['want']['two_systems']
    assert len(set(res['proofs'])) == 4
    assert (res['pad']['arrays'], res['pad']['queries']) == ((0, 0) if mode == 'own_sort' else (2, 2))      # one array per query, none replaced


@pytest.mark.parametrize('mode', ['levels', 'no_levels', 'own_sort'])
def test_two_slot_pipeline_alternates_witnesses(mode, world, shared, shared_no_levels, own_sort):
    """fk_prove_r1cs_submit / _wait over nine steps with four witnesses: the next proof's early front sorts on L's lane, which waits for the
    event behind A's last read of the sort it borrowed"""
    res = dict(levels=shared, no_levels=shared_no_levels, own_sort=own_sort)[mode]['pipeline']
    assert res['direct'] == world['want']['wit']
    assert res['got'] == [world['want']['wit'][i] for i in res['order']]
    assert res['pad']['in_place'] == (mode != 'own_sort')


@pytest.mark.parametrize('mode', ['levels', 'no_levels', 'own_sort'])
def test_foreign_proof_while_the_sort_is_lent(mode, world, shared, shared_no_levels, own_sort):
    """an early front is outstanding -- A's aux part begun on L's sort, its accumulation still deferred (lent_pending > 0) -- when a foreign proof
    arrives: it is refused (or, if the library drops the front instead, proved), and the waiting ticket and the proofs after it are right.
    (msm_abandon itself is reached only from error paths inside a run, which no test can provoke from outside.)"""
    res = dict(levels=shared, no_levels=shared_no_levels, own_sort=own_sort)[mode]['abandon']
    w = world['want']['wit']
    assert res['first'] == w[0] and res['second'] == w[1] and res['third'] == w[2]
    assert (res['foreign'] == w[2]) if res['refused'] is None else (res['refused'][0] == 1 and 'early front' in res['refused'][1])


@pytest.mark.parametrize('mode', ['levels', 'no_levels'])
def test_proofs_after_trim_and_after_a_failed_call(mode, world, shared, shared_no_levels):
    res = dict(levels=shared, no_levels=shared_no_levels)[mode]['recovery']
    assert res['want'] == world['want']['wit'][0]
    assert res['after_trim'] == res['want']
    assert res['error'] is not None and res['error'][0] == 6, res['error']         # FK_ERR_KEY_MISMATCH: the A query of that system does not fit the key
    assert res['after_error'] == res['want']
    assert res['pad']['in_place']


def test_sharded_key_keeps_its_own_sort(world, shared):
    """shards 0 / 2 and 1 / 2 of the key hold half of a and of l each: the precondition fails, A sorts for itself, and the two records fold
    to the unsharded proof"""
    res = shared['sharded']
    assert res['folded'] == res['want'] == world['want']['wit'][0]
    assert all(not p['in_place'] for p in res['pads'])


@pytest.mark.parametrize('same_query', [True, False], ids=['one_query', 'two_queries'])
def test_contexts_in_threads_start_on_a_cold_key(oracle, world, same_query):
    """several contexts, one per host thread, prove from ONE key that no proof has touched yet (include/fawkes_hip.h allows it): their first
    proofs all want the padded array at once.  It is built once per query under the key's lock and never replaced, so every thread gets the
    oracle's bytes -- with one resident system, and with two systems whose A queries differ (both arrays then live side by side)."""
    import threading
    import fixtures as fx
    import fawkes_crypto_amd as fk
    from helpers import r1cs_product
    prev = os.environ.get('FK_MSM_PRE_MIN_LOG2')
    os.environ['FK_MSM_PRE_MIN_LOG2'] = sc.ENV['FK_MSM_PRE_MIN_LOG2']      # levels at this size; read per call by the key loader (the schedule switch is per process: left alone)
    try:
        n = world['n_mid']
        arrays = dict(np.load(os.path.join(world['kdir'], '%d-alternating.npz' % n)))
        prods = [r1cs_product(sc.system(n, sc.density('alternating', n, TILE), seed=n)), r1cs_product(sc.system(n, sc.second_density(n, TILE), seed=n + 7))]
        z = sc.witness('random', n, seed=n + 1)
        r, s = fx.mont_fr(sc.R_S[0]), fx.mont_fr(sc.R_S[1])
        want = [world['want']['two_systems'][0], world['want']['two_systems'][1]]
        ctxs = [fk.Context(0) for _ in range(4)]
        key = ctxs[0].load_key(fk.Parameters(arrays, prods[0]))
        drs = [ctxs[0].load_r1cs(p) for p in prods]
        which = [0, 0, 0, 0] if same_query else [0, 1, 0, 1]
        got, errs = {}, []
        gate = threading.Barrier(len(ctxs))

        def work(i):
            try:
                gate.wait()
                got[i] = [bytes(ctxs[i].prove_witness(key, drs[which[i]], z, r, s)).hex() for _ in range(4)]
            except Exception as e:      # noqa: BLE001
                errs.append(repr(e))

        th = [threading.Thread(target=work, args=(i,)) for i in range(len(ctxs))]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        for i in range(len(ctxs)):
            assert got[i] == [want[which[i]]] * 4, 'context %d' % i
        for d in drs:
            d.free()
        key.free()
        for c in ctxs:
            c.close()
    finally:
        if prev is None:
            os.environ.pop('FK_MSM_PRE_MIN_LOG2', None)
        else:
            os.environ['FK_MSM_PRE_MIN_LOG2'] = prev
