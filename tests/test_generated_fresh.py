"""The committed generated device arithmetic is what its generators write today.

csrc/mont_mul_gfx950.inc and csrc/addsub_gfx950.inc are committed outputs of tools/gen_mont_mul.py and tools/gen_addsub.py.  A
generator edited without regenerating (or an .inc edited by hand) would leave the device code and its description apart; each
generator is therefore run into a temporary directory and its bytes compared with the committed file.  The generators' own static
check of the SGPR-carry hazard rule must have looked at every carry read and found no violation.
"""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'fawkes-crypto_amd', 'csrc')


def _load(name):
    spec = importlib.util.spec_from_file_location('_fresh_' + name, os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize('gen,inc,least', [('gen_mont_mul', 'mont_mul_gfx950.inc', 2000), ('gen_addsub', 'addsub_gfx950.inc', 200)])
def test_generated_file_is_current(gen, inc, least, tmp_path, capsys):
    mod = _load(gen)
    assert os.path.normpath(mod.OUT) == os.path.normpath(os.path.join(CSRC, inc))      # the default still is the committed file
    out = tmp_path / inc
    checked, violations = mod.main(str(out))
    assert violations == 0
    assert checked >= least, 'the hazard check looked at %d carry reads: it no longer sees the generated statements' % checked
    assert '0 violations' in capsys.readouterr().out
    with open(os.path.join(CSRC, inc), 'rb') as f:
        committed = f.read()
    assert out.read_bytes() == committed, '%s is not what tools/%s.py writes: regenerate it' % (inc, gen)
