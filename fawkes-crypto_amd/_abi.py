"""
The C ABI of libfawkes_hip.so as ctypes sees it: the structs and ONE prototype per function of include/fawkes_hip.h.

`load_library()` (api.py) applies the whole table once, so a call with an argument too few, a float for a count or a numpy array for a
pointer raises `ctypes.ArgumentError` / `TypeError` before the library is entered, and plain Python values are converted to the declared
width.  tests/test_ffi_mirror.py compares the table with the header argument by argument, and checks that api.py calls every entry.

Conventions: the five struct out-/in-parameters are typed pointers; every other pointer -- opaque handles, device pointers, host arrays,
strings going in -- is `c_void_p`; `void` functions have restype None; no function has an `errcheck` (callers read the return code).
"""
import ctypes as C

I, U32, U64, Z, D, P, S = C.c_int, C.c_uint32, C.c_uint64, C.c_size_t, C.c_double, C.c_void_p, C.c_char_p


class KeyDesc(C.Structure):
    _fields_ = [('m', C.c_uint64), ('num_input', C.c_uint32), ('num_aux', C.c_uint32),
                ('alpha_g1', C.c_void_p), ('beta_g1', C.c_void_p), ('delta_g1', C.c_void_p),
                ('beta_g2', C.c_void_p), ('delta_g2', C.c_void_p),
                ('h', C.c_void_p), ('n_h', C.c_uint64), ('l', C.c_void_p), ('n_l', C.c_uint64),
                ('a', C.c_void_p), ('n_a', C.c_uint64),
                ('b_g1', C.c_void_p), ('b_g2', C.c_void_p), ('n_b', C.c_uint64),
                ('shard_index', C.c_uint32), ('shard_count', C.c_uint32),
                ('z_frac_lo', C.c_double), ('z_frac_hi', C.c_double)]


class Timings(C.Structure):
    _fields_ = [(n, C.c_double) for n in ('upload_ms', 'ntt_ms', 'msm_h_ms', 'msm_l_ms', 'msm_a_ms', 'msm_b1_ms',
                                          'msm_b2_ms', 'assemble_ms', 'total_ms')]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class R1csStruct(C.Structure):
    _fields_ = [('num_input', C.c_uint32), ('num_aux', C.c_uint32), ('num_gates', C.c_uint64),
                ('a_ptr', C.c_void_p), ('a_col', C.c_void_p), ('a_val', C.c_void_p),
                ('b_ptr', C.c_void_p), ('b_col', C.c_void_p), ('b_val', C.c_void_p),
                ('c_ptr', C.c_void_p), ('c_col', C.c_void_p), ('c_val', C.c_void_p)]


class MsmPlanInfo(C.Structure):
    """fk_msm_plan_info: the window plan of one multiplication and the compile-time limits it is sized against"""
    _fields_ = [('n', C.c_uint64), ('chunk', C.c_uint64)] + [(f, C.c_uint32) for f in (
        'c', 'W', 'B', 'cb', 'wide', 'nchunks', 'cap', 'L', 'T', 'nblk', 'LB', 'nhi', 'nlo',
        's1_tile', 's2_tile', 's2_max_hi', 'over_max', 'seg_min', 'seg_max', 'size_bins')]


class MsmDynInfo(C.Structure):
    """fk_msm_dyn_info: what the front of a multiplication decided on the device"""
    _fields_ = [(f, C.c_uint32) for f in ('cap', 'n_over', 'seg', 'n_tasks', 'n_obs', 'error')] + [('adds', C.c_uint64)]


KEY, TM, CS = C.POINTER(KeyDesc), C.POINTER(Timings), C.POINTER(R1csStruct)

PROTOTYPES = {}          # name -> (restype, argtypes), in the header's order of sections


def _decl(names, restype, *argtypes):
    """functions of one signature share an entry"""
    for name in names.split():
        assert name not in PROTOTYPES, name
        PROTOTYPES[name] = (restype, argtypes)


# ---- context, device buffers, witness slots
_decl('fk_init', I, I, P)
_decl('fk_free', None, P)
_decl('fk_last_error', S, P)
_decl('fk_trim fk_sync fk_stats_reset', I, P)
_decl('fk_set_window_bits', I, P, C.c_uint)
_decl('fk_dev_alloc fk_host_alloc', I, P, Z, P)
_decl('fk_dev_free fk_host_free fk_stream', I, P, P)
_decl('fk_upload fk_download fk_dev_copy', I, P, P, P, Z)
_decl('fk_witness_upload_async', I, P, I, P, Z)
_decl('fk_witness_ptr', I, P, I, P)
_decl('fk_witness_slot', I, P, I, Z, P, P)
_decl('fk_witness_upload_part_async', I, P, I, P, Z, Z)
_decl('fk_witness_mark_ready', I, P, I)
# ---- proving key
_decl('fk_key_load', I, P, KEY, P)
_decl('fk_key_synthetic', I, P, U64, U32, U32, U64, U64, U64, U32, U32, D, D, P)
_decl('fk_key_shard_info fk_key_shard_info2 fk_key_precomputed fk_key_levels_plan fk_key_load_profile fk_key_vk fk_key_counts', I, P, P)   # (key, out[])
_decl('fk_key_derive_levels fk_key_drop_levels', I, P, P)
_decl('fk_key_levels_headroom', I, P, P, P)
_decl('fk_key_host_vk', I, P, P, P, P, P, P)
_decl('fk_key_free', None, P, P)
_decl('fk_key_download', I, P, P, I, P, Z)
_decl('fk_key_load_bellman', I, P, P, Z, U32, U32, U32, D, D, P, P, P, U32, P)
_decl('fk_key_write_bellman', I, P, P, P, P, U32, P, Z, P)
_decl('fk_setup', I, P, CS, P, P, P, P, P, U32, U32, D, D, P, P, P)
_decl('fk_setup_tiled', I, P, CS, U32, P, P, P, P, P, U32, U32, D, D, P, P, P)
# ---- the prover and its multi-rank pieces
_decl('fk_prove fk_prove_dev', I, P, P, P, P, P, U64, P, P, P, P, P, P, P, TM)
_decl('fk_prove_msms fk_prove_msms_dev', I, P, P, P, P, P, U64, P, P, P, P, P, TM)
_decl('fk_prove_msms_z_dev', I, P, P, P, P, P, P, P, TM)
_decl('fk_prove_msm_h_dev fk_prove_msms_finish_dev', I, P, P, P, P)
_decl('fk_prove_msm_array_dev', I, P, P, I, P, P)
_decl('fk_prove_msms_z_begin_dev', I, P, P, P, P, P, P)
_decl('fk_prove_msms_hz_dev', I, P, P, P, P, P, P, P, P, TM)
_decl('fk_prove_assemble', I, P, P, P, U32, P, P, P)
_decl('fk_shard_range fk_h_shard_range', None, U64, U32, U32, P, P)
_decl('fk_work_shard_ranges', None, U64, U64, U64, U32, U32, P)
_decl('fk_work_shard_ranges_q0', None, U64, U64, U64, U64, U32, U32, P)
_decl('fk_dq_gather_dev', I, P, P, U64, U32, U32, U32, P)
_decl('fk_dq_local_dev', I, P, P, P, P, U32, U32, U32, I)
_decl('fk_dq_cross_dev', I, P, P, U32, U32, U32, I)
_decl('fk_dq_cross_sub_dev', I, P, P, P, U32, U32, U32)
# ---- building blocks
_decl('fk_fr_mul_batch', I, P, P, P, P, Z)
_decl('fk_ntt fk_ntt_dev', I, P, P, U32, I, I)
_decl('fk_quotient_h fk_quotient_h_dev', I, P, P, P, P, U64, P)
_decl('fk_msm_g1 fk_msm_g2 fk_msm_g1_dev fk_msm_g2_dev', I, P, P, P, Z, P)
_decl('fk_gen_points_g1_dev fk_gen_points_g2_dev', I, P, P, Z, U64)
_decl('fk_gen_scalars_dev', I, P, P, Z, U64, I)
_decl('fk_msm_plan', I, Z, C.c_uint, I, C.POINTER(MsmPlanInfo))
_decl('fk_msm_front_dump', I, P, P, Z, I, P, P, P, P, P, C.POINTER(MsmDynInfo), P, Z, P, Z)
# ---- synthesis, the resident constraint system, proofs from a witness
_decl('fk_synthesize', I, P, CS, P, P, P, P, P, P, P)
_decl('fk_r1cs_load', I, P, CS, P)
_decl('fk_r1cs_load_tiled', I, P, CS, U32, P)
_decl('fk_r1cs_load_coded', I, P, CS, P, P, P, P, U64, P)
_decl('fk_r1cs_load_gates', I, P, P, P)
_decl('fk_r1cs_free', None, P, P)
_decl('fk_r1cs_info fk_r1cs_density_ptrs', I, P, P)
_decl('fk_r1cs_windows', I, P, P, P, P)
_decl('fk_r1cs_eval_dev', I, P, P, P, P, P, P)
_decl('fk_r1cs_eval_slice_dev', I, P, P, P, U32, U32, U32, P, P, P)
_decl('fk_prove_r1cs fk_prove_r1cs_dev', I, P, P, P, P, P, P, P, TM)
_decl('fk_prove_msms_hz_r1cs_dev', I, P, P, P, P, P, P)
_decl('fk_prove_msms_z_begin_r1cs_dev', I, P, P, P, P)
_decl('fk_prove_r1cs_submit', I, P, P, P, P, P, P, P)
_decl('fk_prove_r1cs_wait', I, P, I, P, TM)
# ---- gate blobs
_decl('fk_gates_decode', I, P, P, Z, I, U32, U32, U32, P)
_decl('fk_gates_free fk_blob_free', None, P)
_decl('fk_gates_info fk_gates_profile fk_blob_profile', I, P, P)
_decl('fk_gates_export', I, P, I, P, P, P)
_decl('fk_gates_encode', I, P, CS, U32, I, I, I, P)
_decl('fk_blob_data', I, P, P, P)
# ---- N GPUs behind one call
_decl('fk_init_devices', I, I, P, P)
_decl('fk_multi_free', None, P)
_decl('fk_multi_last_error fk_multi_transport', S, P)
_decl('fk_multi_size fk_multi_sync', I, P)
_decl('fk_multi_topology fk_multi_witness_traffic', I, P, P)
_decl('fk_multi_preflight', I, P, Z, P, P, P)
_decl('fk_multi_ctx fk_multi_key_shard fk_multi_r1cs_replica', P, P, I)
_decl('fk_multi_key_load', I, P, KEY, P)
_decl('fk_multi_key_load_bellman', I, P, P, Z, U32, P, P, P, U32, P)
_decl('fk_multi_setup', I, P, CS, P, P, P, P, P, P, P, P)
_decl('fk_multi_setup_tiled', I, P, CS, U32, P, P, P, P, P, P, P, P)
_decl('fk_multi_key_free fk_multi_r1cs_free', None, P, P)
_decl('fk_multi_r1cs_load', I, P, CS, P)
_decl('fk_multi_r1cs_load_tiled', I, P, CS, U32, P)
_decl('fk_multi_r1cs_load_gates', I, P, P, P)
_decl('fk_multi_prove_r1cs', I, P, P, P, P, P, P, P, TM)
_decl('fk_multi_prove_r1cs_submit', I, P, P, P, P, P, P, P)
_decl('fk_multi_prove_r1cs_wait', I, P, I, P, TM)
# ---- verifier
_decl('fk_verify', I, P, P, Z, P, U32, P, P)
_decl('fk_verify_batch_dev', I, P, P, Z, P, U32, P, U32, P)
# ---- Poseidon, JubJub, EdDSA-Poseidon
_decl('fk_poseidon_params_new', I, U32, U32, U32, P, P)
_decl('fk_poseidon_params_load', I, U32, U32, U32, P, P, P)
_decl('fk_poseidon_params_get', I, P, P, P, P)
_decl('fk_poseidon_free', None, P)
_decl('fk_poseidon_hash_batch fk_poseidon_hash_batch_dev', I, P, P, P, U32, Z, P)
_decl('fk_poseidon_sponge_batch', I, P, P, P, U64, Z, P)
_decl('fk_poseidon_merkle_tree_dev fk_poseidon_merkle_root', I, P, P, P, U64, P)
_decl('fk_poseidon_merkle_proofs_dev', I, P, P, U32, P, Z, P)
_decl('fk_poseidon_merkle_proof_roots fk_poseidon_merkle_proof_roots_dev', I, P, P, P, P, P, U32, Z, P)
_decl('fk_jubjub_params fk_eddsa_hash_r', I, P, P, P)
_decl('fk_jubjub_mul_batch', I, P, P, P, Z, P)
_decl('fk_jubjub_decompress_batch', I, P, P, Z, P, P)
_decl('fk_eddsa_sign_batch', I, P, P, P, P, P, Z, P, P, P)
_decl('fk_eddsa_verify_batch fk_eddsa_verify_batch_dev', I, P, P, P, P, P, P, Z, P)
# ---- statistics, tracing
_decl('fk_roctx_active', I)
_decl('fk_calibrate', I, P, P)
_decl('fk_stats_get', I, P, I, P, P, P)

# entry points api.py does not wrap (bench.py and the tools call them through load_library()); tests/test_ffi_mirror.py holds api.py to this list
NOT_WRAPPED = ('fk_roctx_active',)


def apply(lib):
    """sets restype / argtypes of every table entry on a loaded library; a symbol the library lacks is an error that names it"""
    for name, (restype, argtypes) in PROTOTYPES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise AttributeError('libfawkes_hip.so does not export %s (declared in include/fawkes_hip.h): rebuild the library' % name) from None
        fn.restype, fn.argtypes = restype, list(argtypes)
