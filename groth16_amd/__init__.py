"""groth16_amd -- MI355X-native Groth16 prover hot path behind ark-groth16's prover API.

Host-side mirror (Python, because no Rust toolchain exists in this image) of the reference's
prover interface for the accelerated path; everything below the method signatures goes through
the C ABI of ``libg16_mi355x.so`` (include/g16_mi355x.h) -- there is no CPU fallback.

Reference interface mirrored (paths relative to /root/reference):
  Groth16.create_proof_with_reduction_and_matrices   src/prover.rs:26-51
  Groth16.create_proof_with_reduction_no_zk          src/prover.rs:155-168 (matrices form)
  Groth16.create_random_proof_with_reduction         src/prover.rs:138-150 (matrices form)
  LibsnarkReduction.witness_map_from_matrices        src/r1cs_to_qap.rs:172-235
  Groth16(curve, device, qap=...) / CircomReduction  trait R1CSToQAP, src/r1cs_to_qap.rs:71-120 (Groth16<E, QAP>); the second
      implementor is ark-circom's, restated from its published source
  ProvingKey / Proof / ConstraintMatrices            src/data_structures.rs:8-16,125-143
  SynthesisError.PolynomialDegreeTooLarge            src/r1cs_to_qap.rs:178-179
  Groth16.generate_parameters_with_qap               src/generator.rs:47-208 (matrices form)
  Groth16.generate_parameters_from_srs / contribute_delta / group_ntt, SRS
                                                    generator.rs:129-183, r1cs_to_qap.rs:120-170, 236-246 with points for scalars: a key
      from a powers-of-tau SRS, nobody holding tau, alpha or beta (host twins: generate_parameters_from_srs_host, group_ntt_host)
  Groth16.rlc_sums / check_srs / check_delta_contribution / check_parameters, generate_parameters_from_srs(check=True), BadSRS
                                                    no counterpart in the reference (a ceremony's verifier, snarkjs' `zkey verify`; libg16_ceremony.so):
      is the SRS a sequence of powers, does a key descend from it -- pairings over random linear combinations, the sums on the GPU
      (host twins: rlc_sums_host, check_srs_host, check_delta_contribution_host)
  Groth16.batch_scalar_mul / contribute_tau / check_tau_contribution / phase1_timings, TauContribution
                                                    no counterpart in the reference (phase 1 of a ceremony, snarkjs' `powersoftau contribute` /
      `verify` without their files and proofs of knowledge; libg16_phase1.so): one scalar per point on the GPU, a contribution to
      the powers of tau, its check (host twins: batch_scalar_mul_host, contribute_tau_host, check_tau_contribution_host)
  Groth16.check_key_derivation / fold_key_from_srs / keycheck_timings, check_parameters(derive=False)
                                                    no counterpart in the reference (snarkjs' `zkey verify` without re-deriving the key;
      libg16_keycheck.so): random linear combinations pushed through the matrices and the scalar transform onto the SRS -- the
      prover's row walk, transforms and MSMs, no transform over the group (host twins: check_key_derivation_host, fold_key_from_srs_host)
  Groth16.prepare_srs / generate_parameters_from_lagrange / group_ntt_windowed / lagrange_timings, LagrangeSRS (save / load)
                                                    no counterpart in the reference (snarkjs' `powersoftau prepare phase2`; libg16_lagrange.so):
      the Lagrange form of an SRS made once per domain, every circuit's key from it by the sparse products alone; the transforms on
      phase 1's windowed scalar multiplication (host twins: prepare_srs_host, generate_parameters_from_lagrange_host,
      group_ntt_windowed_host)
  rerandomize_proof / Groth16.rerandomize_proof      src/prover.rs:223-250 (host: three scalar multiplications)
  Groth16.create_proof_with_reduction / prove / setup src/prover.rs:173-217, src/lib.rs:63-82, src/generator.rs:20-45 -- host-side
      synthesis (groth16_amd.r1cs: ConstraintSystem, Variable, lc, ConstraintSynthesizer) in front of the GPU calls
  Groth16.prepare_verifying_key / prepare_inputs / verify_proof_with_prepared_inputs / verify_proof, process_vk /
      verify_with_processed_vk                      src/verifier.rs:13-76, src/lib.rs:84-96 (GPU batch: verify_proofs)
  VerifyingKey / PreparedVerifyingKey               src/data_structures.rs:31-66
  Groth16.check_assignment / is_satisfied / which_is_unsatisfied, host_check_assignment, ConstraintSystem.which_is_unsatisfied,
      check=True on create_proof* / prove / PipelinedProver.submit, Unsatisfiable
                                                    debug_assert!(cs.is_satisfied().unwrap()), src/prover.rs:193 (ark-relations'
      is_satisfied / which_is_unsatisfied, SynthesisError::Unsatisfiable) -- kept in "release": the check runs on the GPU
"""
from .binding import (G16Error, Lib, PolynomialDegreeTooLarge, SynthesisError, UnexpectedIdentity, lib, FQ_LIMBS, CURVE_ID)  # noqa: F401
from .groth16 import (CheckResult, CircomReduction, ConstraintMatrices, DeviceProvingKey, Groth16, LibsnarkReduction, PipelinedProver, Proof, ProvingKey, ShardedProver, finalize_host,  # noqa: F401
                      host_check_assignment, rerandomize_proof, shard_ranges, SRS, group_ntt_host, generate_parameters_from_srs_host,
                      BadSRS, CeremonyResult, rlc_plan, rlc_sums_host, check_srs_host, check_delta_contribution_host,
                      TauContribution, batch_scalar_mul_host, contribute_tau_host, check_tau_contribution_host,
                      check_key_derivation_host, fold_key_from_srs_host,
                      LagrangeSRS, group_ntt_windowed_host, prepare_srs_host, generate_parameters_from_lagrange_host)
from .binding import InvalidData, MalformedVerifyingKey, Unsatisfiable  # noqa: F401
from .verifier import (PreparedVerifyingKey, VerifyingKey, check_subgroups_host, decompress_points_host, host_pairing, verify_proof_host,  # noqa: F401
                       verify_proofs_aggregate_host, verify_proofs_aggregate_mixed_host, decode_points_host)
from .r1cs import AssignmentMissing, ConstraintSynthesizer, ConstraintSystem, LinearCombination, Variable, lc  # noqa: F401

__all__ = [
    "Groth16", "LibsnarkReduction", "CircomReduction", "ConstraintMatrices", "ProvingKey", "Proof", "ShardedProver", "PipelinedProver", "G16Error", "SynthesisError",
    "PolynomialDegreeTooLarge", "UnexpectedIdentity", "lib", "ConstraintSystem", "ConstraintSynthesizer", "Variable", "LinearCombination",
    "lc", "AssignmentMissing", "VerifyingKey", "PreparedVerifyingKey", "MalformedVerifyingKey", "verify_proof_host", "verify_proofs_aggregate_host", "verify_proofs_aggregate_mixed_host", "check_subgroups_host", "host_pairing",
    "decompress_points_host", "CheckResult", "Unsatisfiable", "host_check_assignment", "DeviceProvingKey", "InvalidData", "decode_points_host",
    "SRS", "group_ntt_host", "generate_parameters_from_srs_host",
    "BadSRS", "CeremonyResult", "rlc_plan", "rlc_sums_host", "check_srs_host", "check_delta_contribution_host",
    "TauContribution", "batch_scalar_mul_host", "contribute_tau_host", "check_tau_contribution_host",
    "check_key_derivation_host", "fold_key_from_srs_host",
    "LagrangeSRS", "group_ntt_windowed_host", "prepare_srs_host", "generate_parameters_from_lagrange_host",
]
