"""Test infrastructure: records the witness program of a circuit of oracle/fawkes_circuit.py while the circuit is built.

    with witness_trace.trace() as t:
        cs, _ = fc.poseidon_merkle_circuit(leaf, sibling, path, depth=2)
    prog, given = t.program(cs)          # a fawkes_crypto_amd.witness.WitnessProgram and the instance's given row

Inside the block the four functions of the circuit DSL that allocate a COMPUTED variable are wrapped; a call that makes `cs.num_aux` grow
has allocated, and what it allocated is recorded against the new variable(s):
    CNum.mul            -> MUL  <self> <other>                        (num.rs:247-262)
    c_div_unchecked     -> DIV0 <a> <b>                               (num.rs:37-47)
    c_is_zero           -> INV0 <a> on the FIRST new variable; the two products behind it record themselves  (num.rs:65-79)
    c_into_bits_le      -> BIT <signal> i on the limit - 1 consecutive variables, i = 1 .. limit - 1          (bitify.rs:9-48)
CS.inputize records the combination of each public input.  Every other allocation is GIVEN, in allocation order: the value the caller of
the circuit supplies (public values, secrets, path bits, cofactor preimages).  The originals are restored on exit; nothing under oracle/
is edited."""
import contextlib

import fawkes_circuit as fc
from fawkes_crypto_amd import witness as W


def _terms(n):
    """a CNum's combination as ((column, coefficient), ...) in the reference's term order: column 0 = ONE, 1 + j = Aux(j)"""
    out = []
    for kind, idx in sorted(n.lc):
        assert kind == 1 or idx == 0, 'a combination names the public input %d' % idx
        out.append((1 + idx if kind else 0, n.lc[(kind, idx)]))
    return tuple(out)


class Trace:
    def __init__(self):
        self._ops, self._public = {}, {}

    def _record(self, cs, var, rec):
        self._ops.setdefault(id(cs), {})[var] = rec

    def program(self, cs):
        """(WitnessProgram, given row) of one traced CS"""
        ops = self._ops.get(id(cs), {})
        p, given, lc_id = W.WitnessProgram(), [], {}

        def lc(terms):                      # the same tuple object is recorded once per signal: intern by identity first
            i = lc_id.get(id(terms))
            if i is None:
                i = lc_id[id(terms)] = p.lc(terms)
            return i

        for v in range(cs.num_aux):
            rec = ops.get(v)
            if rec is None:
                assert p.given() == v
                given.append(cs.z_aux[v])
            elif rec[0] == W.MUL:
                assert p.mul(lc(rec[1]), lc(rec[2])) == v
            elif rec[0] == W.DIV0:
                assert p.div0(lc(rec[1]), lc(rec[2])) == v
            elif rec[0] == W.INV0:
                assert p.inv0(lc(rec[1])) == v
            else:
                assert p.bit(lc(rec[1]), rec[2]) == v
        for terms in self._public.get(id(cs), []):
            p.public(lc(terms))
        assert p.num_input == cs.num_input and p.num_aux == cs.num_aux
        return p, given


@contextlib.contextmanager
def trace():
    t = Trace()
    orig = (fc.CNum.mul, fc.c_div_unchecked, fc.c_is_zero, fc.c_into_bits_le, fc.CS.inputize)

    def mul(self, o):
        cs, n0 = self.cs, self.cs.num_aux
        res = orig[0](self, o)
        if cs.num_aux > n0:
            assert cs.num_aux == n0 + 1
            t._record(cs, n0, (W.MUL, _terms(self), _terms(o)))
        return res

    def div_unchecked(a, b):
        cs, n0 = a.cs, a.cs.num_aux
        res = orig[1](a, b)
        if cs.num_aux > n0:
            assert cs.num_aux == n0 + 1
            t._record(cs, n0, (W.DIV0, _terms(a), _terms(b)))
        return res

    def is_zero(a):
        cs, n0 = a.cs, a.cs.num_aux
        res = orig[2](a)
        if cs.num_aux > n0:
            t._record(cs, n0, (W.INV0, _terms(a)))
        return res

    def into_bits_le(signal, limit):
        cs, n0 = signal.cs, signal.cs.num_aux
        res = orig[3](signal, limit)
        if cs.num_aux > n0:
            assert cs.num_aux == n0 + limit - 1
            terms = _terms(signal)
            for i in range(1, limit):
                t._record(cs, n0 + i - 1, (W.BIT, terms, i))
        return res

    def inputize(self, n):
        t._public.setdefault(id(self), []).append(_terms(n))
        return orig[4](self, n)

    fc.CNum.mul, fc.c_div_unchecked, fc.c_is_zero, fc.c_into_bits_le, fc.CS.inputize = mul, div_unchecked, is_zero, into_bits_le, inputize
    try:
        yield t
    finally:
        fc.CNum.mul, fc.c_div_unchecked, fc.c_is_zero, fc.c_into_bits_le, fc.CS.inputize = orig
