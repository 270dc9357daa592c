"""The witness program on the host (no GPU): tracing the circuits of oracle/fawkes_circuit.py (tests/witness_trace.py), the Python-integer
interpreter `WitnessProgram.run_host` against the witness the circuit builder itself computed, the host-side check of the C ABI
(fk_witness_program_check) on good and on hand-broken programs, and include/fawkes_hip_witness.h against the library and the ctypes
table of fawkes_crypto_amd/witness.py.  Every comparison is exact."""
import ctypes as C
import os
import random
import re
import subprocess
import tempfile

import numpy as np
import pytest

import bn254_ref as ref
import fawkes_circuit as fc
import fixtures as fx
import witness_trace
import fawkes_crypto_amd as fk
from fawkes_crypto_amd import witness as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'fawkes_hip_witness.h')
FK_ERR_BAD_ARG, FK_ERR_FORMAT = 1, 7


def merkle_instances(depth, n, seed=11):
    rnd = random.Random(seed)
    return [fc.poseidon_merkle_circuit(rnd.randrange(ref.R), [rnd.randrange(ref.R) for _ in range(depth)], [rnd.randrange(2) for _ in range(depth)], depth)[0]
            for _ in range(n)]


def eddsa_instance(seed=4096):
    rnd = random.Random(seed)
    return fc.eddsa_circuit(rnd.randrange(fc.FS), rnd.randrange(ref.R), rnd.randrange(fc.FS))[0]


def rollup_instance(depth=2, seed=2025):
    rnd = random.Random(seed)
    return fc.rollup_tx_circuit(rnd.randrange(fc.FS), 500, 400, [rnd.randrange(ref.R) for _ in range(depth)], [rnd.randrange(2) for _ in range(depth)],
                                rnd.randrange(fc.FS), depth)


@pytest.fixture(scope='module')
def traced():
    """name -> (list of CS, list of (program, given row)), traced once for the module"""
    out = {}
    with witness_trace.trace() as t:
        made = {'merkle2': merkle_instances(2, 3), 'merkle32': merkle_instances(32, 1), 'eddsa': [eddsa_instance()], 'rollup2': [rollup_instance()]}
    for name, css in made.items():
        out[name] = (css, [t.program(cs) for cs in css])
    return out


# aux, GIVEN, MUL, DIV0, INV0, BIT, runs of BITs that share one combination
COUNTS = {'merkle32': (7394, 66, 7328, 0, 0, 0, 0), 'merkle2': (464, 6, 458, 0, 0, 0, 0),
          'eddsa': (4119, 8, 2740, 611, 4, 756, 4), 'rollup2': (5498, 15, 4112, 611, 4, 756, 4)}


@pytest.mark.parametrize('name', sorted(COUNTS))
def test_traced_program_reproduces_the_circuit_witness(traced, name):
    css, progs = traced[name]
    for cs, (p, given) in zip(css, progs):
        c = p.counts()
        assert (p.num_aux, c['GIVEN'], c['MUL'], c['DIV0'], c['INV0'], c['BIT'], c['BIT_runs']) == COUNTS[name]
        assert p.n_given == c['GIVEN'] == len(given)
        z = p.run_host([given])
        assert z[:p.num_input] == cs.z_in and z[p.num_input:] == cs.z_aux
        assert cs.satisfied()
        W.check(p)
    # one gadget, one program: the instances differ in their given rows only
    p0 = progs[0][0]
    assert all((p.op, p.arg0, p.arg1, p.input_lc, p.lcs) == (p0.op, p0.arg0, p0.arg1, p0.input_lc, p0.lcs) for p, _ in progs[1:])


def test_trace_restores_the_circuit_dsl():
    before = (fc.CNum.mul, fc.c_div_unchecked, fc.c_is_zero, fc.c_into_bits_le, fc.CS.inputize)
    with pytest.raises(ZeroDivisionError):
        with witness_trace.trace():
            assert fc.CNum.mul is not before[0]
            1 / 0
    assert (fc.CNum.mul, fc.c_div_unchecked, fc.c_is_zero, fc.c_into_bits_le, fc.CS.inputize) == before


def test_three_copies_come_out_in_the_tiled_order(traced):
    from test_gpu_tiled import _tile_z
    css, progs = traced['merkle2']
    p = progs[0][0]
    picks = [2, 0, 1]
    zs = [fx.witness_mont(cs.z_in, cs.z_aux) for cs in css]
    assert len({tuple(cs.z_in) for cs in css}) == 3
    want = _tile_z(zs, p.num_input, picks)
    got = fk.api._fr_rows(p.run_host([progs[k][1] for k in picks]))
    assert got.shape == want.shape == (p.witness_len(3), 4) and np.array_equal(got, want)


# ---------------------------------------------------------------- fk_witness_program_check
def small_program():
    """g0, g1 given; v2 = g0 * g1; v3 = (g0 + 3) / v2; v4 = 1 / v3; v5, v6 = bits 0, 5 of g1 + 2 v2; one public input v4 + ONE"""
    p = W.WitnessProgram()
    g0, g1 = p.given(), p.given()
    v2 = p.mul(p.lc([(1 + g0, 1)]), p.lc([(1 + g1, 1)]))
    v3 = p.div0(p.lc([(1 + g0, 1), (0, 3)]), p.lc([(1 + v2, 1)]))
    v4 = p.inv0(p.lc([(1 + v3, 1)]))
    bits = p.lc([(1 + g1, 1), (1 + v2, 2)])
    p.bit(bits, 0)
    p.bit(bits, 5)
    p.public(p.lc([(1 + v4, 1), (0, 1)]))
    return p


def test_small_program_runs_and_passes_the_check():
    p = small_program()
    W.check(p)
    W.check(p.desc(explicit_ones=True))
    R = ref.R
    z = p.run_host([[5, 7], [0, 9]])
    v2, v3 = 35, 8 * pow(35, -1, R) % R
    v4 = pow(v3, -1, R)
    assert z == [1, (v4 + 1) % R, 1,
                 5, 7, v2, v3, v4, (7 + 70) & 1, ((7 + 70) >> 5) & 1,
                 0, 9, 0, 0, 0, 1, 0]           # 3 / 0 = 0, 1 / 0 = 0, bits of 9


def _refused(desc, code, *names):
    with pytest.raises(fk.FkError) as e:
        W.check(desc)
    assert e.value.code == code, str(e.value)
    for n in names:
        assert n in str(e.value), str(e.value)


def test_check_refuses_each_violation():
    def broken(edit):
        p = small_program()
        edit(p)
        return p

    def set_(attr, i, v):
        return lambda p: getattr(p, attr).__setitem__(i, v)

    _refused(broken(set_('op', 2, 5)), FK_ERR_BAD_ARG, 'variable 2', 'opcode')
    _refused(broken(set_('op', 6, 255)), FK_ERR_BAD_ARG, 'variable 6', 'opcode')
    _refused(broken(set_('arg1', 2, 99)), FK_ERR_BAD_ARG, 'variable 2', 'combination 99')             # a combination index >= n_lc
    _refused(broken(set_('arg0', 4, 7)), FK_ERR_BAD_ARG, 'variable 4', 'combination 7')
    _refused(broken(lambda p: p.input_lc.__setitem__(0, 8)), FK_ERR_BAD_ARG, 'input 1', 'combination 8')
    _refused(broken(lambda p: p.lcs.__setitem__(3, ((1 + 7, 1),))), FK_ERR_BAD_ARG, 'combination 3', 'column 8')      # a column > num_aux
    _refused(broken(lambda p: p.lcs.__setitem__(3, ((1 + 4, 1),))), FK_ERR_BAD_ARG, 'variable 3', 'combination 3', 'Aux(4)')   # a later variable
    _refused(broken(lambda p: p.lcs.__setitem__(3, ((1 + 3, 1),))), FK_ERR_BAD_ARG, 'variable 3', 'combination 3', 'Aux(3)')   # its own variable
    _refused(broken(lambda p: p.lcs.__setitem__(0, ((1 + 2, 1),))), FK_ERR_BAD_ARG, 'variable 2', 'combination 0', 'Aux(2)')
    _refused(broken(set_('arg1', 6, 256)), FK_ERR_BAD_ARG, 'variable 6', 'bit index 256')
    _refused(broken(set_('arg0', 1, 2)), FK_ERR_BAD_ARG, 'variable 1', 'given index 2')
    # the descriptor itself
    d = small_program().desc()
    d.keep[4][2] = int(d.keep[4][1]) - 1
    _refused(d, FK_ERR_BAD_ARG, 'lc_ptr', 'combination 1')
    d = small_program().desc()
    d.keep[4][0] = 1
    _refused(d, FK_ERR_BAD_ARG, 'lc_ptr')
    d = small_program().desc()
    d.num_input = 0
    _refused(d, FK_ERR_BAD_ARG, 'num_input')
    d = small_program().desc()
    d.op = None
    _refused(d, FK_ERR_BAD_ARG, 'missing')
    d = small_program().desc()
    d.keep[6][3] = fk.api.int_to_limbs(ref.R)               # the image r itself: one past the largest
    _refused(d, FK_ERR_FORMAT, 'combination 2', 'term 1')
    d = small_program().desc()
    d.keep[6][3] = fk.api.int_to_limbs(ref.R - 1)
    W.check(d)
    # a public input may name any variable, an operation may name the variable right before it
    p = small_program()
    p.public(p.lc([(p.num_aux, 1)]))
    p.mul(p.lc([(p.num_aux, 1)]), p.lc([(p.num_aux, 5), (0, 1)]))
    W.check(p)


def test_an_empty_program_is_valid():
    p = W.WitnessProgram()
    W.check(p)
    assert p.run_host([[], []]) == [1]


# ---------------------------------------------------------------- the header, the library, the ctypes table
def _declared():
    text = re.sub(r'/\*.*?\*/', ' ', open(HEADER).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r'\b(fk_\w+)\s*\(([^()]*)\)\s*;', text):
        out[name] = len([a for a in args.split(',') if a.strip() and a.strip() != 'void'])
    return out


def test_header_compiles_alone_as_c99():
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, 'alone.c')
        open(src, 'w').write('#include "fawkes_hip_witness.h"\nint main(void) { fk_witness_desc d; (void)d; return FK_WOP_BIT == 4 ? 0 : 1; }\n')
        subprocess.check_call(['gcc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), src, '-o', os.path.join(td, 'alone')])
        subprocess.check_call([os.path.join(td, 'alone')])


def test_every_declared_function_is_exported_and_prototyped():
    decl = _declared()
    assert sorted(decl) == sorted(W.PROTOTYPES) and len(decl) == 6
    lib = fk.load_library()
    for name, nargs in decl.items():
        assert hasattr(lib, name), name
        assert len(W.PROTOTYPES[name][1]) == nargs, name
    # kept out of the pinned ABI and of api.py
    assert not any(n.startswith('fk_witness_program') or n.startswith('fk_witness_generate') for n in fk.EXPORTED_SYMBOLS)
    assert '.fk_witness_program' not in open(os.path.join(ROOT, 'fawkes-crypto_amd', 'api.py')).read()


def test_descriptor_layout_c_vs_ctypes():
    fields = [f[0] for f in W.WitnessDesc._fields_]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "fawkes_hip_witness.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(fk_witness_desc));']
    prog += ['  printf("%s %%zu\\n", offsetof(fk_witness_desc, %s));' % (f, f) for f in fields]
    prog += ['  return 0;', '}']
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, 'layout.c'), os.path.join(td, 'layout')
        open(src, 'w').write('\n'.join(prog))
        subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), src, '-o', exe])
        got = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    assert int(got.pop('size')) == C.sizeof(W.WitnessDesc)
    assert {f: int(v) for f, v in got.items()} == {f: getattr(W.WitnessDesc, f).offset for f in fields}
