#!/bin/bash
# the whole GPU suite, smoke(), the whole benchmark (--full).  Output: ${OUT:-out}/final/
O=${OUT:-out}/final; mkdir -p $O
python3 -m pytest tests -m gpu -q --durations=8 > $O/pytest_gpu.log 2>&1; echo "pytest rc=$?" >> $O/pytest_gpu.log; tail -3 $O/pytest_gpu.log
python3 -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $O/smoke.log 2>&1; tail -1 $O/smoke.log
( time python3 bench.py --full ) > $O/bench.log 2> $O/bench.err; tail -c 600 $O/bench.log; grep real $O/bench.err
