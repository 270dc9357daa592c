"""Child of tests/test_gpu_spmv_dedup.py: proves the explicit system of 4 rollup-style transactions of the committed fixture (block-sorted,
with row windows) under the environment it was started with -- once through fk_prove_r1cs (the chunked hand-over: one evaluation per
window) and once through fk_prove_r1cs_submit / _wait -- and prints the aliases in force and the proof bytes.  FK_SPMV_DEDUP is read once
per process, hence the subprocess."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bench  # noqa: E402  (data loading helpers only; nothing of the oracle)
import fawkes_crypto_amd as fk  # noqa: E402

copies = 4
ctx = fk.Context(0)
n_in, n_aux, mats, table = bench.materialise_rollup(copies)
inst, zs = bench.load_rollup_instance()
z = bench.tile_witness(zs[:3], inst.num_input, copies)
dr = ctx.load_r1cs_coded(n_in, n_aux, mats, table)
assert dr.windows() is not None
info = (C.c_uint64 * 4)()
fn = ctx.lib.fk_r1cs_alias_info
fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
assert fn(dr.handle, info) == 0
tox = {k: bench.mont(v) for k, v in bench.TOXIC.items()}
key, vk = ctx.setup(inst, copies=copies, **tox)          # the tiled set-up describes the same rows and variables
r, s = bench.mont(0xA11CE), bench.mont(0xB0B)
chunked = bytes(ctx.prove_witness(key, dr, z, r, s)).hex()
ticket = ctx.prove_witness_submit(key, dr, z, r, s)
piped = bytes(ctx.prove_witness_wait(ticket)).hex()
print('PROOFS', int(info[0]), chunked, piped)
