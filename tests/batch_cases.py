"""Cases shared by tests/test_batch_plan_host.py and tests/test_gpu_batch_prove.py (the batch prover, include/fawkes_hip_batch.h)."""
import numpy as np

import bn254_ref as ref
import fixtures as fx

R = ref.R

# ---------------------------------------------------------------- the plan sweep
PLAN_LOG_M = range(1, 21)
PLAN_COUNTS = (1, 2, 63, 64, 65, 1000)
PLAN_BUDGETS = (1 << 20, 1 << 28, 1 << 36)          # less than one proof of a large domain needs; a few proofs; room for every count


def plan_queries(m):
    """query lengths of a key with domain m, in the proportions of BASELINE configs[0] (m = 2^13: l 7359, a 7230, b 2817)"""
    return max(1, m * 9 // 10), max(1, m * 88 // 100), max(1, m * 34 // 100)


# ---------------------------------------------------------------- witness layouts
def tile_rows(zs, num_input):
    """witness rows (count, nv, 4) -> the tiled order: ONE, every proof's inputs, every proof's aux"""
    zs = [np.asarray(z, np.uint64).reshape(-1, 4) for z in zs]
    return np.ascontiguousarray(np.concatenate([zs[0][:1]] + [z[1:num_input] for z in zs] + [z[num_input:] for z in zs]))


def mont_rows(values):
    """canonical ints -> (n, 4) uint64 Montgomery"""
    return fx.co.limbs_arr([ref.to_mont(int(v) % R, R) for v in values]) if len(values) else np.zeros((0, 4), np.uint64)


# ---------------------------------------------------------------- scalar rows of the multiplication tests
MSM_FORCED_BITS = (2, 14)           # FK_BATCH_WINDOW_BITS_MIN, _MAX


def msm_scalar_rows(n, count, rng):
    """`count` rows of n canonical-int scalars, cycling through: a witness-like row (zeros, ones, uniform), a uniform row, all 0, all 1,
    all r - 1, and 2^(c k), 2^(c k) - 1 for both forced window widths c (digit boundaries and carries).  count = 1 gets the witness-like
    row, 3 adds uniform and all-zero, 65 goes through all nine seven times."""
    from helpers import mont_ints, rand_fr_mont

    def pow_row(c, minus):
        return [((1 << (c * ((j + i) % (254 // c) + 1))) - minus) % R for j in range(n)]

    rows = []
    for i in range(count):
        k = i % 9
        if k == 0:
            rows.append(mont_ints(rand_fr_mont(rng, n, kind='witness')))
        elif k == 1:
            rows.append(mont_ints(rand_fr_mont(rng, n)))
        elif k < 5:
            rows.append([(0, 1, R - 1)[k - 2]] * n)
        else:
            rows.append(pow_row(MSM_FORCED_BITS[(k - 5) // 2], (k - 5) % 2))
    return rows
