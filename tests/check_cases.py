"""Shared by tests/test_r1cs_check_host.py and tests/test_gpu_r1cs_check.py: what the R1CS check must report, from the oracle alone
(`c_oracle.synthesize` plus `fe_mul_batch`, never the code under test), and witnesses that violate chosen gates."""
import random

import numpy as np

import bn254_ref as ref
import c_oracle as co
import fixtures as fx

R = ref.R
NONE = (1 << 64) - 1
GROUP_ROWS = (1, 64)


class Want:
    """the expected report of a witness all of whose images are below r"""

    def __init__(self, csr, z, group_rows=0):
        G = csr.num_gates
        a, b, c = (x[:G] for x in co.synthesize(csr, z)[:3])
        bad = np.flatnonzero((co.fe_mul_batch(co.FR, a, b) != c).any(axis=1)) if G else np.zeros(0, np.int64)
        self.gates, self.bad = G, [int(g) for g in bad]
        self.n_bad = len(self.bad)
        self.first_bad = self.bad[0] if self.bad else NONE
        self.first_abc = np.stack([a[bad[0]], b[bad[0]], c[bad[0]]]) if self.bad else np.zeros((3, 4), np.uint64)
        self.bitmap = np.zeros((G + 63) // 64, np.uint64)
        for g in self.bad:
            self.bitmap[g >> 6] |= np.uint64(1 << (g & 63))
        self.group_rows = group_rows
        self.n_groups = (G + group_rows - 1) // group_rows if group_rows else 0
        self.flags = np.zeros(self.n_groups, np.uint8)
        if group_rows:
            self.flags[sorted({g // group_rows for g in self.bad})] = 1
        self.n_bad_groups = int(self.flags.sum())
        self.one_ok = int(np.array_equal(z[0], fx.mont_fr(1)))

    def regroup(self, group_rows):
        w = Want.__new__(Want)
        w.__dict__.update(self.__dict__)
        w.group_rows = group_rows
        w.n_groups = (self.gates + group_rows - 1) // group_rows if group_rows else 0
        w.flags = np.zeros(w.n_groups, np.uint8)
        if group_rows:
            w.flags[sorted({g // group_rows for g in self.bad})] = 1
        w.n_bad_groups = int(w.flags.sum())
        return w


def struct_fields(st):
    """a fk_check_report as a comparable dict"""
    return dict(gates=int(st.gates), n_bad=int(st.n_bad), first_bad=int(st.first_bad), first_abc=[[int(x) for x in row] for row in st.first_abc],
                n_groups=int(st.n_groups), n_bad_groups=int(st.n_bad_groups), n_range=int(st.n_range), first_range=int(st.first_range),
                one_ok=int(st.one_ok), gates_valid=int(st.gates_valid))


def want_fields(w):
    return dict(gates=w.gates, n_bad=w.n_bad, first_bad=w.first_bad, first_abc=[[int(x) for x in row] for row in w.first_abc],
                n_groups=w.n_groups, n_bad_groups=w.n_bad_groups, n_range=0, first_range=NONE, one_ok=w.one_ok, gates_valid=1)


def assert_report(rep, w):
    """a fawkes_crypto_amd.check.CheckReport against the oracle's expectation: every field, the bitmap, the flags"""
    assert rep.gates == w.gates and rep.n_bad == w.n_bad
    assert rep.first_bad == (None if w.first_bad == NONE else w.first_bad)
    assert np.array_equal(rep.first_abc_mont, w.first_abc)
    if w.bad:
        assert list(rep.first_abc) == [ref.from_mont(x, R) for x in co.ints(w.first_abc)]
    else:
        assert rep.first_abc is None
    assert (rep.n_groups, rep.n_bad_groups) == (w.n_groups, w.n_bad_groups)
    assert (rep.n_range, rep.first_range, rep.one_ok, rep.gates_valid) == (0, None, bool(w.one_ok), True)
    assert rep.ok == (w.n_bad == 0 and bool(w.one_ok))
    assert np.array_equal(rep.bitmap(), w.bitmap)
    assert [int(g) for g in rep.bad_rows()] == w.bad
    if w.group_rows:
        assert np.array_equal(rep.group_flags(), w.flags)
        assert [int(k) for k in rep.bad_groups()] == [int(k) for k in np.flatnonzero(w.flags)]


def bad_gates(csr, z):
    return set(Want(csr, z).bad)


def violate(csr, z, gates, seed=1):
    """A copy of z in which every gate of `gates` is violated, by altering witness elements that gate reads: the first variable of its A
    row, then (where B's value is zero, so that the product stays zero) the variables of its B row -- never ONE.  One altered variable
    may break other gates too: what is bad afterwards is the oracle's to say."""
    rnd = random.Random(seed)
    z = np.array(z, copy=True)
    for g in gates:
        cand = [int(csr.A.col[int(csr.A.ptr[g])])] + [int(v) for v in csr.B.col[int(csr.B.ptr[g]):int(csr.B.ptr[g + 1])]]
        for v in cand:
            if v == 0:
                continue
            z[v] = fx.mont_fr(rnd.randrange(2, R))
            if g in bad_gates(csr, z):
                break
        else:
            raise AssertionError('gate %d could not be violated' % g)
    return z


def all_bad(csr, z, seed=2):
    """every variable but ONE redrawn: every gate of a fast_r1cs system is then violated (checked)"""
    rnd = random.Random(seed)
    z = np.array(z, copy=True)
    z[1:] = co.limbs_arr([ref.to_mont(rnd.randrange(2, R), R) for _ in range(len(z) - 1)])
    assert len(bad_gates(csr, z)) == csr.num_gates
    return z


def bad_sets(gates):
    """the violated gates of the explicit-system cases: gate 0; 63 and 64 together; the last gate (where the system has them)"""
    sets = [[0], [gates - 1]] if gates > 1 else [[0]]
    if gates > 64:
        sets.append([63, 64])
    if gates > 2:
        sets.append(sorted({0, min(63, gates - 2), gates - 1}))
    return sets


def explicit_case(gates, seed=None):
    """(R1csC, its satisfying witness)"""
    csr, z, _, _ = fx.fast_r1cs(seed if seed is not None else 900 + gates, gates, 3, gates + 7)
    return csr, z


def tiled_case(G, copies):
    """(the instance, the explicit system of `copies` of it, the satisfying tiled witness)"""
    inst, _, z_in, z_aux = fx.fast_r1cs(700 + G, G, 3, G + 5)
    return inst, fx.tile_r1cs(inst, copies), fx.tile_witness([z_in] * copies, [z_aux] * copies)


def violate_copies(inst, full, z, copies_bad, seed=3):
    """gate 2 (mod G) of every copy of `copies_bad` violated; only that copy's own variables are altered, so exactly these copies are bad"""
    G = inst.num_gates
    z = violate(full, z, [k * G + min(2, G - 1) for k in copies_bad], seed)
    assert {g // G for g in bad_gates(full, z)} == set(copies_bad)
    return z
