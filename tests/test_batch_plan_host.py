"""The batch prover without a GPU: the plan's invariants over every domain size (fk_prove_batch_plan is host only), the refusals that
need no context, and include/fawkes_hip_batch.h against the library and the ctypes table of fawkes-crypto_amd/batch.py, argument by argument."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

import fawkes_crypto_amd as fk
from fawkes_crypto_amd import batch as B
from batch_cases import PLAN_BUDGETS, PLAN_COUNTS, PLAN_LOG_M, plan_queries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'fawkes_hip_batch.h')
FK_ERR_BAD_ARG = 1


# ---------------------------------------------------------------- plan
@pytest.mark.parametrize('budget', PLAN_BUDGETS)
def test_plan_invariants(budget):
    for log_m in PLAN_LOG_M:
        m = 1 << log_m
        launches = set()
        for count in PLAN_COUNTS:
            p = B.plan(m, *plan_queries(m), count, dict(scratch_budget_bytes=budget))
            where = (log_m, count, budget, p)
            assert 1 <= p['group'] <= B.MAX_GROUP, where
            assert p['group'] * p['n_groups'] >= count > p['group'] * (p['n_groups'] - 1), where
            assert p['scratch_bytes'] <= budget or p['group'] == 1, where
            for bits, windows in ((p['window_bits_g1'], p['windows_g1']), (p['window_bits_g2'], p['windows_g2'])):
                assert B.WINDOW_BITS_MIN <= bits <= B.WINDOW_BITS_MAX, where
                assert windows * bits >= 254, where
            assert p['segment'] >= 1 and p['ntt_passes'] == (log_m + 8) // 9, where
            launches.add(p['launches_per_group'])
        assert len(launches) == 1 and launches.pop() > 0, (log_m, budget)       # the launches of a group do not depend on count


def test_plan_group_grows_with_the_budget_and_a_group_of_one_is_always_allowed():
    m = 1 << 13
    q = plan_queries(m)
    groups = [B.plan(m, *q, 1000, dict(scratch_budget_bytes=b))['group'] for b in (1, 1 << 24, 1 << 28, 1 << 32, 1 << 40)]
    assert groups == sorted(groups) and groups[0] == 1 and groups[-1] == 1000
    tight = B.plan(1 << 20, *plan_queries(1 << 20), 5, dict(scratch_budget_bytes=1))
    assert tight['group'] == 1 and tight['n_groups'] == 5 and tight['scratch_bytes'] > 1
    assert B.plan(m, *q, 0)['n_groups'] == 0
    # default budget of the host-only plan, as the header states it
    assert B.plan(m, *q, 64)['scratch_bytes'] <= B.PLAN_DEFAULT_BUDGET


def test_plan_forced_window_bits_are_kept():
    m = 1 << 10
    for c in (B.WINDOW_BITS_MIN, 7, B.WINDOW_BITS_MAX):
        p = B.plan(m, *plan_queries(m), 8, dict(window_bits_g1=c, window_bits_g2=c))
        assert (p['window_bits_g1'], p['window_bits_g2']) == (c, c) and p['windows_g1'] == 254 // c + 1
    both = B.plan(m, *plan_queries(m), 8, dict(window_bits_g1=6, window_bits_g2=9))
    same = B.plan(m, *plan_queries(m), 8, dict(window_bits_g1=6, window_bits_g2=6))
    assert both['launches_per_group'] > same['launches_per_group']         # B2 sorts for itself when its width differs from B1's


@pytest.mark.parametrize('m,opts,said', [(3, None, 'power of two'), (0, None, 'power of two'), (1, None, 'power of two'), (12288, None, 'power of two'),
                                         (1 << 21, None, 'fk_prove_r1cs_dev'),
                                         (1 << 10, dict(window_bits_g1=1), 'window bits'), (1 << 10, dict(window_bits_g1=15), 'window bits'),
                                         (1 << 10, dict(window_bits_g2=1), 'window bits'), (1 << 10, dict(window_bits_g2=23), 'window bits')])
def test_plan_refusals(m, opts, said):
    with pytest.raises(fk.FkError) as e:
        B.plan(m, *plan_queries(max(m, 2)), 4, opts)
    assert e.value.code == FK_ERR_BAD_ARG and said in str(e.value)


def test_plan_null_out_and_entries_without_a_context():
    lib = B._lib()
    assert lib.fk_prove_batch_plan(1 << 10, 10, 10, 10, 1, None, None) == FK_ERR_BAD_ARG
    out = (C.c_uint8 * 256)()
    rs = (C.c_uint64 * 4)()
    # no context: refused before anything is touched, whatever else is null
    assert lib.fk_prove_batch_dev(None, None, None, None, 0, 1, rs, rs, out, None, None) == FK_ERR_BAD_ARG
    assert lib.fk_prove_batch_dev(None, None, None, None, 0, 0, None, None, None, None, None) == FK_ERR_BAD_ARG
    assert lib.fk_prove_batch(None, None, None, None, 1, rs, rs, out, None, None) == FK_ERR_BAD_ARG
    assert lib.fk_batch_r1cs_eval_dev(None, None, None, 0, 1, None, None, None) == FK_ERR_BAD_ARG
    assert lib.fk_batch_quotient_dev(None, None, None, None, 2, 1, 1, None) == FK_ERR_BAD_ARG
    assert lib.fk_batch_msm_dev(None, None, 1, 0, None, 0, None, 0, 1, 1, 1, None, None) == FK_ERR_BAD_ARG
    assert bytes(out) == bytes(256)


# ---------------------------------------------------------------- the header, the library, the ctypes table
STRUCTS = {'fk_batch_opts': B.BatchOpts, 'fk_batch_plan_info': B.BatchPlanInfo, 'fk_batch_timings': B.BatchTimings}
C_INTS = {'int': (True, 4), 'int32_t': (True, 4), 'uint32_t': (False, 4), 'uint64_t': (False, 8), 'size_t': (False, 8), 'unsigned': (False, 4)}


def _strip(text):
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    return '\n'.join(l for l in text.splitlines() if not l.strip().startswith('#'))


def _c_kind(ty):
    """'const fk_batch_opts *' -> ('ptr', 'fk_batch_opts'); 'const void *' -> ('ptr', None); 'uint32_t' -> ('int', False, 4)"""
    depth = ty.count('*')
    base = ' '.join(re.sub(r'\b(const|struct)\b', ' ', ty.replace('*', ' ')).split())
    if depth:
        return ('ptr', base if base in STRUCTS else None)
    if base == 'double':
        return ('f64',)
    return ('int',) + C_INTS[base]


def _py_kind(t):
    if t is C.c_void_p:
        return ('ptr', None)
    if isinstance(t, type) and issubclass(t, C._Pointer):
        return ('ptr', {v: k for k, v in STRUCTS.items()}[t._type_])
    if t is C.c_double:
        return ('f64',)
    return ('int', t(-1).value < 0, C.sizeof(t))


def parse_header(text):
    text = _strip(text)
    text = re.sub(r'typedef\s+struct\s*\{.*?\}\s*\w+\s*;', ' ', text, flags=re.S)
    funcs = {}
    for m in re.finditer(r'([\w\s\*]+?)\b(fk_\w+)\s*\(([^;{}]*?)\)\s*;', text, flags=re.S):
        params = []
        for a in m.group(3).split(','):
            a = re.sub(r'\[.*?\]', '*', a.strip())
            mm = re.match(r'(.*?)(\w+)\s*(\**)$', a, flags=re.S)
            params.append((mm.group(2), _c_kind(mm.group(1) + mm.group(3))))
        funcs[m.group(2)] = (_c_kind(m.group(1)), params)
    return funcs


def _problems(funcs, table):
    out = ['%s is declared in the header and missing from the table' % n for n in funcs if n not in table]
    for name, (restype, argtypes) in table.items():
        if name not in funcs:
            out.append('%s is in the table and not declared in the header' % name)
            continue
        ret, params = funcs[name]
        if _py_kind(restype) != ret:
            out.append('%s returns %s, the header says %s' % (name, _py_kind(restype), ret))
        if len(argtypes) != len(params):
            out.append('%s takes %d arguments, the header %d' % (name, len(argtypes), len(params)))
            continue
        for t, (pn, pk) in zip(argtypes, params):
            if _py_kind(t) != pk:
                out.append('%s argument %s is %s, the header has %s' % (name, pn, _py_kind(t), pk))
    return out


def test_prototype_table_mirrors_the_header_argument_by_argument():
    funcs = parse_header(open(HEADER).read())
    assert len(funcs) == 6 and set(funcs) == set(B.PROTOTYPES)
    assert _problems(funcs, B.PROTOTYPES) == []
    lib = fk.load_library()
    for name in funcs:
        assert hasattr(lib, name), name
    # kept out of the pinned ABI and of api.py
    assert not any(n.startswith('fk_prove_batch') or n.startswith('fk_batch_') for n in fk.EXPORTED_SYMBOLS)
    assert '.fk_prove_batch' not in open(os.path.join(ROOT, 'fawkes-crypto_amd', 'api.py')).read()
    # negative control: a narrower integer, an untyped struct pointer, a dropped argument and a missing function are each reported
    ret, args = B.PROTOTYPES['fk_prove_batch_plan']
    for bad, said in (((ret, (C.c_uint32,) + args[1:]), 'fk_prove_batch_plan argument m is'), ((ret, args[:-1] + (C.c_void_p,)), 'fk_prove_batch_plan argument out is'),
                      ((ret, args[:-1]), 'fk_prove_batch_plan takes 6 arguments, the header 7'), (None, 'fk_prove_batch_plan is declared in the header and missing')):
        table = dict(B.PROTOTYPES)
        if bad is None:
            del table['fk_prove_batch_plan']
        else:
            table['fk_prove_batch_plan'] = bad
        problems = _problems(funcs, table)
        assert len(problems) == 1 and problems[0].startswith(said), (said, problems)


def test_header_compiles_alone_as_c99_and_the_constants_agree():
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, 'alone.c')
        open(src, 'w').write('#include "fawkes_hip_batch.h"\nint main(void) { fk_batch_opts o; (void)o; return FK_BATCH_Z_ROWS == %d && FK_BATCH_Z_TILED == %d '
                             '&& FK_BATCH_MAX_LOG_M == %d && FK_BATCH_WINDOW_BITS_MIN == %d && FK_BATCH_WINDOW_BITS_MAX == %d && FK_BATCH_MAX_GROUP == %d '
                             '&& FK_BATCH_PLAN_DEFAULT_BUDGET == %dull ? 0 : 1; }\n'
                             % (B.Z_ROWS, B.Z_TILED, B.MAX_LOG_M, B.WINDOW_BITS_MIN, B.WINDOW_BITS_MAX, B.MAX_GROUP, B.PLAN_DEFAULT_BUDGET))
        subprocess.check_call(['gcc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-Wno-long-long', '-I', os.path.join(ROOT, 'include'), src, '-o', os.path.join(td, 'alone')])
        subprocess.check_call([os.path.join(td, 'alone')])


def test_struct_layouts_c_vs_ctypes():
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "fawkes_hip_batch.h"', 'int main(void) {']
    for s, cls in STRUCTS.items():
        prog.append('  printf("%s size %%zu\\n", sizeof(%s));' % (s, s))
        prog += ['  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (s, f[0], s, f[0]) for f in cls._fields_]
    prog += ['  return 0;', '}']
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, 'layout.c'), os.path.join(td, 'layout')
        open(src, 'w').write('\n'.join(prog))
        subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), src, '-o', exe])
        got = {}
        for line in subprocess.check_output([exe], text=True).splitlines():
            s, f, v = line.split()
            got.setdefault(s, {})[f] = int(v)
    for s, cls in STRUCTS.items():
        assert got[s].pop('size') == C.sizeof(cls), s
        assert got[s] == {f[0]: getattr(cls, f[0]).offset for f in cls._fields_}, s
