"""
fawkes-crypto_amd -- MI355X (gfx950) Groth16 proving backend for fawkes-crypto.

Host-side mirror (ctypes over the C ABI in include/fawkes_hip.h) of the reference interface
`fawkes_crypto::backend::bellman_groth16::{Parameters, prover::{Proof, prove}, group::{G1Point, G2Point}}`
(/root/reference/fawkes-crypto/src/backend/bellman_groth16/{mod.rs:139-175, prover.rs:13-90, group.rs:13-122}).

The directory name carries a hyphen (the reference's crate name); import it as `fawkes_crypto_amd`
(the sibling shim package at the repo root) -- both names load this file.

There is NO CPU fallback: if libfawkes_hip.so is missing or no GPU is visible, `Context()` raises.
"""
from .api import (  # noqa: F401
    FkError, Context, MultiContext, Parameters, Proof, VK, G1Point, G2Point, R1cs, prove, prove_with_rs, lib_path, load_library,
    FK_MSM_RESULT_BYTES, FK_PROOF_BYTES, EXPORTED_SYMBOLS, build_library,
    verify, verify_batch, vk_to_borsh, synthesize, sample_fr, PoseidonParams, MerkleTree,
    jubjub_params, eddsa_hash_r, FS_MODULUS,
)
from . import parallel  # noqa: F401
from . import params_io  # noqa: F401
from . import witness  # noqa: F401
from . import verify_agg  # noqa: F401
from . import check  # noqa: F401
from . import merkle  # noqa: F401
from . import sparse_merkle  # noqa: F401
from .sparse_merkle import SparseMerkleTree  # noqa: F401
from . import merkle_set  # noqa: F401
from . import batch  # noqa: F401
from .batch import prove_batch, prove_batch_dev, prove_given_batch  # noqa: F401
from . import ceremony  # noqa: F401
from . import ceremony_init  # noqa: F401
from .ceremony_init import (  # noqa: F401
    PowersOfTau, PowersReport, g1_ntt, g2_ntt, initial_key, initial_key_host, initial_image, check_powers, check_powers_host,
)
from . import powers  # noqa: F401
from .powers import (  # noqa: F401
    PowersPublic, PointsReport, PowersUpdateReport, new_powers, contribute, contribute_host, scale_powers, scale_powers_dev, validate_points,
    check_update, check_update_host,
)
