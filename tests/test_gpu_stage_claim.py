"""The claim on the context's staging buffers and lanes: while a submitted proof's early front holds them, every entry that borrows them
is refused and the _dev hashing and signature entries keep running (tests/_stage_child.py)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_borrowers_are_refused_during_an_early_front():
    """the early front exists under the sorts-first schedule only, which is chosen per process: tests/_stage_child.py"""
    env = {k: v for k, v in os.environ.items() if not k.startswith(('FK_SPMV_', 'FK_PROVE_'))}
    env['FK_PROVE_SORTS_FIRST'] = '1'
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_stage_child.py')], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert 'STAGE ok refused=True' in out.stdout, out.stdout[-1000:]
