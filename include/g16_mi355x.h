/* g16_mi355x.h -- C ABI of the MI355X-native Groth16 prover hot path.
 *
 * Drop-in boundary for ark-groth16 0.5.0 (paths relative to /root/reference):
 *   g16_prove            <->  Groth16::create_proof_with_reduction_and_matrices   src/prover.rs:26-51
 *                             (= witness_map_from_matrices  src/r1cs_to_qap.rs:172-235
 *                              + create_proof_with_assignment src/prover.rs:54-132)
 *   g16_witness_map      <->  LibsnarkReduction::witness_map_from_matrices        src/r1cs_to_qap.rs:172-235
 *   g16_msm_g1 / _g2     <->  VariableBaseMSM::msm_bigint call sites              src/prover.rs:66,74,262
 *   g16_ntt              <->  EvaluationDomain::{fft,ifft}_in_place (+coset)      src/r1cs_to_qap.rs:201-232
 *   g16_pk_load          <->  &ProvingKey<E>                                      src/data_structures.rs:125-143
 *   g16_circuit_load     <->  &ConstraintMatrices<F>, num_inputs, num_constraints src/prover.rs:30-32
 *   g16_pvk_load         <->  prepare_verifying_key / process_vk                    src/verifier.rs:13-20, src/lib.rs:84-86
 *   g16_verify_batch     <->  verify_proof (per proof)                             src/verifier.rs:25-76
 *   g16_verify_batch_prepared <-> verify_proof_with_prepared_inputs               src/verifier.rs:44-65
 *   g16_circuit_check    <->  cs.is_satisfied() / cs.which_is_unsatisfied() (ark-relations) behind the debug_assert! of
 *                             src/prover.rs:193; g16_prove_checked = that assertion kept in a release build, then g16_prove
 *   g16_prove_partial / g16_prove_finalize: the same proof with the MSM base set sharded
 *                             over several GPUs (one process per GPU; the host exchanges the
 *                             fixed-size g16_partial records, e.g. one RCCL all-gather).
 * The reference has no FFI of its own (#![forbid(unsafe_code)], src/lib.rs:13); INTEGRATION.md
 * shows the Rust binding a maintainer would add.
 *
 * Data conventions (zero conversion on the Rust side):
 *   field element  : arkworks in-memory form -- little-endian u64 limbs of a*R mod p (Montgomery),
 *                    Fr: 4 limbs (both curves); Fq: 6 limbs (BLS12-381) / 4 limbs (BN254)
 *   G1 affine      : x | y              (2*FQ limbs)
 *   G2 affine      : x.c0 x.c1 y.c0 y.c1 (4*FQ limbs)
 *   identity       : all limbs zero (arkworks Affine::identity() has x = y = 0, infinity = true;
 *                    (0,0) is not on either curve, so the flag is redundant)
 *   CSR matrix     : row_ptr u64[num_constraints+1], col u32[nnz], val Fr[nnz]; built from
 *                    ConstraintMatrices' Vec<Vec<(F, usize)>> rows
 * All functions return 0 on success or a g16_status; they never throw or unwind.
 * A g16_ctx is bound to one HIP device (g16_ctx_create) or to several (g16_ctx_create_multi) and is thread-compatible
 * (one call in flight per ctx).  A g16_pk / g16_circuit may be used by every single-device context on the GPU it was loaded on
 * (its device data is read-only during a proof; everything a proof writes belongs to the calling context), from different
 * threads at once: two contexts on one GPU proving side by side over one key is the THROUGHPUT mode -- the head (witness map) and
 * tail (reductions, host glue) of one proof run under the bucket passes of the other (bench.py reports it as `pipelined`).
 * Free a key / circuit only when no call on any context is using it.
 */
#ifndef G16_MI355X_H
#define G16_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    G16_OK = 0,
    G16_ERR_DEGREE_TOO_LARGE = 1, /* SynthesisError::PolynomialDegreeTooLarge (r1cs_to_qap.rs:178-179) */
    G16_ERR_BAD_LENGTH = 2,       /* the reference would panic on a slice bound (prover.rs:44-45)      */
    G16_ERR_BAD_ARG = 3,
    G16_ERR_HIP = 4,
    G16_ERR_OOM = 5,
    G16_ERR_NO_DEVICE = 6,
    G16_ERR_INTERNAL = 7,
    G16_ERR_UNEXPECTED_IDENTITY = 8, /* SynthesisError::UnexpectedIdentity: gamma or delta is zero (generator.rs:110-111) */
    G16_ERR_INVALID_DATA = 9,        /* SerializationError::InvalidData: bytes that are not a point of the group        */
    G16_ERR_NO_PEER_ACCESS = 10,     /* g16_ctx_create_multi with G16_MULTI_REQUIRE_PEER=1: a device pair without peer access */
    G16_ERR_MALFORMED_VK = 11,       /* SynthesisError::MalformedVerifyingKey: public inputs + 1 != gamma_abc_g1 (verifier.rs:29-31) */
    G16_ERR_UNSATISFIED = 12         /* SynthesisError::Unsatisfiable (ark-relations): g16_prove_checked met a row with a*b != c       */
} g16_status;

typedef enum { G16_BLS12_381 = 0, G16_BN254 = 1 } g16_curve;

typedef struct g16_ctx g16_ctx;
typedef struct g16_pk g16_pk;
typedef struct g16_circuit g16_circuit;

/* one query vector (or a contiguous shard of it) */
typedef struct {
    const uint64_t* points; /* affine points, host memory (or device memory if G16_PK_DEVICE_PTRS) */
    uint64_t count;         /* points in this shard                                               */
    uint64_t start;         /* index of points[0] within the logical MSM base array               */
} g16_query;

#define G16_PK_DEVICE_PTRS 1u /* query `points` are device pointers on the ctx's GPU */

/* g16_pk_load never modifies or retains the caller's arrays.  What it keeps on the GPU per query is either the
 * bases (in the bucket kernel's radix) or -- the default -- their WINDOW TABLE: W rows 2^(c j) * query, c = 20 and
 * W = 13 for keys of 2^20 points and more, i.e. 13x the memory of the key (31 GB for 2^22 BLS12-381 constraints),
 * which cuts the prover's dominant kernel by a fifth.  Environment: G16_MSM_PRECOMP=0 keeps plain
 * bases; G16_PK_TABLE_BUDGET_MB caps one query's table; a failed allocation falls back to plain bases. */

/* ProvingKey<E> as the prover reads it (src/data_structures.rs:125-143; vk fields prover.rs:92,105,113).
 * MSM base arrays, in the index space the prover uses:
 *   a, b_g1, b_g2 : query[1..]   (index i <-> full_assignment[1+i]),  logical length m
 *   l             : l_query      (index j <-> full_assignment[num_inputs+j]), logical length w
 *   h             : h_query      (index k <-> h[k]), logical length n-1
 * query[0] of a / b_g1 / b_g2 is passed separately (calculate_coeff, prover.rs:261). */
typedef struct {
    const uint64_t* alpha_g1; /* vk.alpha_g1 */
    const uint64_t* beta_g1;
    const uint64_t* delta_g1;
    const uint64_t* beta_g2;  /* vk.beta_g2  */
    const uint64_t* delta_g2; /* vk.delta_g2 */
    const uint64_t* a_query0;
    const uint64_t* b_g1_query0;
    const uint64_t* b_g2_query0;
    g16_query a, b_g1, b_g2, h, l;
    uint32_t flags;
} g16_pk_view;

typedef struct {
    const uint64_t* row_ptr;
    const uint32_t* col;
    const uint64_t* val;
} g16_csr_view;

/* Proof<E> (src/data_structures.rs:8-16), affine Montgomery limbs; only the first
 * 2*FQ / 4*FQ / 2*FQ limbs of a / b / c are meaningful. */
typedef struct {
    uint64_t a[12];
    uint64_t b[24];
    uint64_t c[12];
} g16_proof;

/* Partial MSM sums of one shard, extended-Jacobian (X, Y, ZZ, ZZZ) Montgomery limbs.
 * Fixed size so that it can be all-gathered as raw bytes. */
typedef struct {
    uint64_t h[24], l[24], a[24], b_g1[24]; /* 4*FQ limbs used */
    uint64_t b_g2[48];                      /* 8*FQ limbs used */
} g16_partial;

/* phase timings of the last g16_prove on this ctx, milliseconds (GPU events + host clock);
 * names follow the reference's timers (prover.rs:36,62,89,99,111,119) */
typedef struct {
    double witness_map_ms; /* for a HOST assignment (assignment_on_device == 0) the upload's pieces land UNDER the map's first kernels, whose
                              row blocks wait for them: the figure then includes the ~2.4 ms (2^22) the 128 MiB take to arrive; with
                              the assignment resident, or G16_UPLOAD_CHUNKED=0 (one copy ahead of the timer), it is the map alone */
    double msm_h_ms, msm_l_ms, msm_a_ms, msm_b_g1_ms, msm_b_g2_ms;
    double scalar_prep_ms; /* into_bigint + digit extraction + bucket sort (shared by the MSMs) */
    double finish_ms;      /* host glue: scalar muls, final adds, into_affine */
    double total_ms;
    double bucket_pass_ms; /* sum over the 5 MSMs of the bucket-accumulation kernel */
    double bucket_ms[5];   /* that kernel per MSM: h, l, a, b_g1 (G1 kernel), b_g2 (G2 kernel); HIP events on the ctx stream (see g1_pass_launches) */
    double window_bits;    /* Pippenger window size c of the witness MSMs in the last call ... */
    double windows;        /* ... and their window count W: a bucket pass folds (bases in the shard) * W points */
    double ntt_ms;         /* the seven transforms of r1cs_to_qap.rs:201-232 alone (inside witness_map_ms, which also covers
                              the three sparse mat-vecs and the pointwise pass) */
    double g1_pass_launches; /* launches of the G1 bucket kernel in the last call: MSMs that are ready together share ONE launch
                              (l, a, b_g1; h too in a sharded proof), bucket_ms[] then holds each one's share of it by points */
} g16_timings;

int g16_ctx_create(int curve, int device_id, g16_ctx** out);
/* One context over n_dev GPUs of the node, so that the reference's single call -- Groth16::prove, src/lib.rs:76-82
 * -> create_proof_with_reduction, src/prover.rs:173-217 -- stays a single g16_prove: g16_pk_load (given the WHOLE key: every
 * query.start == 0, host pointers) cuts the five MSM base arrays into n_dev contiguous shards, one per device;
 * g16_circuit_load replicates the matrices; g16_prove (host full_assignment) runs one host thread per device and folds the
 * n_dev partial records on the host.  When n_dev is a power of two <= 16 with n_dev^2 | domain_size the witness map is
 * distributed as well (the g16_dwm_* stages below on every device, the all-to-all as peer copies between the devices' buffers
 * over xGMI) and g16_pk_load gathers every h_query shard in the block order that leaves h in (the key must then be the
 * circuit's: h_query holds domain_size - 1 bases, generator.rs:168; anything else is G16_ERR_BAD_LENGTH at g16_prove).  g16_prove_partial is the per-device form and is refused on such a context;
 * g16_prove_finalize and the unit-level entry points run on the first device.  device_ids may repeat.  n_dev == 1 is
 * g16_ctx_create.
 * How g16_pk_load cuts the key over the devices (round 5; G16_MULTI_SHARD_MODE=auto|base|bucket, default auto): by BASE RANGES as above, or in
 * BUCKET SPACE (g16_pk_load_bucket_shard on every device: the whole key's window tables per device, device i owns the buckets
 * b mod n_dev == i, and with the distributed witness map every device pulls ALL blocks of h -- the all-gather as peer copies); auto picks
 * bucket space while the whole key's tables stay below 80 GiB and fit in every device's free memory, and falls back to base ranges if
 * such a load then runs out of memory (a FORCED bucket-space load does not fall back: G16_ERR_OOM).  g16_pk_get_info says which.
 * EXPERIMENTAL for n_dev > 1 over distinct devices: every test so far ran with one physical GPU listed several times (the build
 * pool has one-GPU boxes), so peer access, hipMemcpyPeerAsync between devices and the cross-device event waits of g16_prove have
 * not met real hardware; tests/test_gpu_parity.py::test_multi_device_context_distinct_gpus runs wherever >= 2 GPUs are visible.
 * The process-per-GPU form (g16_prove_partial + one all-gather, bench.py --gpus N) is the supported multi-GPU path. */
int g16_ctx_create_multi(int curve, const int* device_ids, int n_dev, g16_ctx** out);
int g16_ctx_num_devices(const g16_ctx* ctx);
/* 1: device i of the context reaches device j's memory directly (hipDeviceCanAccessPeer said yes and the access was enabled, or
 * i and j are the same physical device); 0: copies between the two are staged through host memory by the runtime (correct, slow --
 * G16_MULTI_REQUIRE_PEER=1 makes g16_ctx_create_multi fail with G16_ERR_NO_PEER_ACCESS instead); -1: bad index. */
int g16_ctx_peer_access(const g16_ctx* ctx, int i, int j);
void g16_ctx_destroy(g16_ctx* ctx);
/* HIP stream the ctx launches on (hipStream_t); lets callers bracket work with their own events */
void* g16_ctx_stream(g16_ctx* ctx);

int g16_pk_load(g16_ctx* ctx, const g16_pk_view* view, g16_pk** out);
void g16_pk_free(g16_pk* pk);

/* BUCKET-SPACE SHARD of the five MSMs (src/prover.rs:66,74,262) over `world` ranks, the second way to cut them (the first: base
 * ranges, g16_query.start / count above).  Every rank loads the WHOLE key (`view` as for one GPU: every query.start == 0) as
 * window tables -- 31 GB at 2^22 BLS12-381 constraints, 126 GB at 2^24: what 288 GB of HBM per GPU are for -- and owns the buckets
 * b with  b mod world == rank  of the merged-window bucket set (interleaved, so that the short top window's entries spread
 * evenly).  A rank's sort keeps only the (point, window) entries of its residue class, its bucket passes fold ~1/world of them
 * at the full window size (c = 20, W = 13, ~100 entries per bucket), and -- the point of the mode -- its bucket REDUCTIONS shrink
 * world-fold too, which a base-range shard's do not (every rank keeps all 2^(c-1) buckets of all five MSMs there).  With local
 * index k = b / world:  sum_{b owned} (b+1) S_b = world * sum_k (k+1) S_k + (rank + 1 - world) * sum_k S_k.
 * g16_prove_partial / g16_prove_partial_h over such a key yield the rank's partial sums; the exchange (one all-gather of the
 * g16_partial records) and g16_prove_finalize are unchanged.  The scalars are needed WHOLE on every rank: the assignment as for
 * one GPU, and h either from the replicated witness map (g16_prove_partial) or -- distributed map -- all-gathered (n Fr; the
 * ranks' blocks back to back, h_query loaded in that same order) and passed to g16_prove_partial_h.
 * No silent fall-back: G16_ERR_OOM if the whole key's tables do not fit, G16_ERR_BAD_ARG for a key that cannot have tables
 * (G16_MSM_PRECOMP=0) or a view that is itself a base-range shard.  world == 1 is g16_pk_load. */
int g16_pk_load_bucket_shard(g16_ctx* ctx, const g16_pk_view* view, int rank, int world, g16_pk** out);
/* The resident tables do not depend on the rank: re-label a whole key held as window tables (g16_pk_load, or a bucket-space shard)
 * as rank `rank` of `world` (world == 1: the whole bucket set again).  Not while a call is using the key.  Lets one GPU walk through
 * every rank's share (parity tests at 2^24, bench.py --sim-shards); a base-range shard or a plain-bases key is G16_ERR_BAD_ARG. */
int g16_pk_rebind_bucket_shard(g16_pk* pk, int rank, int world);

/* How a loaded key is held (no reference counterpart).  table_fallback says WHY a key is held as plain bases -- a slower prover:
 * per-window buckets, c <= 16, more windows -- instead of window tables: 0 window tables (the default);
 * 1 plain bases by request (G16_MSM_PRECOMP=0); 2 a query too long for merged entries; 3 the tables did not fit next to what
 * already lives on the GPU (allocation failed, or G16_PK_TABLE_BUDGET_MB). */
typedef struct {
    int window_bits_z;      /* window size c of the witness MSMs' tables (0: plain bases)  */
    int window_bits_h;      /* ... of h_query's                                          */
    int table_fallback;     /* reason code above                                         */
    int bucket_shard_rank;  /* g16_pk_load_bucket_shard: rank, world (0, 1 otherwise)    */
    int bucket_shard_world;
    int n_devices;          /* 1, or the devices of a multi-device key (fields above: device 0's shard) */
    uint64_t device_bytes;  /* HBM held by the five query arrays (per device)            */
} g16_pk_info;
int g16_pk_get_info(const g16_pk* pk, g16_pk_info* out);

/* num_variables = num_instance_variables + num_witness_variables (len of full_assignment) */
int g16_circuit_load(g16_ctx* ctx, const g16_csr_view abc[3], uint64_t num_inputs, uint64_t num_constraints,
                     uint64_t num_variables, g16_circuit** out);
/* ---- the R1CS -> QAP reduction (trait R1CSToQAP, src/r1cs_to_qap.rs:71-120; Groth16<E, QAP>) ----
 * G16_QAP_LIBSNARK: the reference's LibsnarkReduction -- h = coefficients of (A.B - C) / Z, h_query = domain_size - 1 bases.
 * G16_QAP_CIRCOM:   ark-circom's CircomReduction (snarkjs-compatible keys), restated from its published source and NOT pinned
 *                   against it: rows as above but c = a .* b (the C matrix is not read), each of a, b, c through ifft, times rho^i
 *                   (rho the generator of the 2n-point domain, rho^2 = w), fft; h[i] = a[i] b[i] - c[i] -- the n evaluations of
 *                   A.B - C on the odd coset, natural order, no division by Z.  h_query = domain_size bases, the odd-indexed
 *                   entries of the size-2n inverse transform of delta^-1 t^i (i < 2n - 1).  G16_ERR_DEGREE_TOO_LARGE if 2n exceeds
 *                   the field's two-adicity.
 * g16_circuit_load is g16_circuit_load_qap with qap = 0.  A Circom circuit keeps A and B on the device only: abc[2] may be all-NULL.
 * Refused with G16_ERR_BAD_ARG: a Circom circuit on a multi-device context, and g16_dwm_create over a Circom circuit (the multi-device
 * key loader gathers h_query in the distributed map's block order before it knows the circuit).  Everything else -- g16_witness_map
 * (still domain_size Fr out), g16_prove, g16_prove_partial over base-range and bucket-space shards, g16_prove_finalize -- follows the
 * circuit's reduction.  A key must come from the same reduction: a Circom circuit proved with a Libsnark key of the same circuit
 * passes the length rules (domain_size - 1 <= domain_size bases) and yields a proof the verifier rejects. */
typedef enum { G16_QAP_LIBSNARK = 0, G16_QAP_CIRCOM = 1 } g16_qap;
int g16_circuit_load_qap(g16_ctx* ctx, const g16_csr_view abc[3], uint64_t num_inputs, uint64_t num_constraints,
                         uint64_t num_variables, int qap, g16_circuit** out);
int g16_circuit_qap(const g16_circuit* c); /* g16_qap of a loaded circuit; -1 for NULL */
void g16_circuit_free(g16_circuit* c);
uint64_t g16_circuit_domain_size(const g16_circuit* c);

/* full_assignment: n_assign Fr (host memory unless assignment_on_device != 0); r, s: one Fr each */
int g16_prove(g16_ctx* ctx, const g16_pk* pk, const g16_circuit* circuit, const uint64_t* full_assignment,
              uint64_t n_assign, int assignment_on_device, const uint64_t r[4], const uint64_t s[4], g16_proof* out);

/* ---- R1CS satisfaction on the GPU: debug_assert!(cs.is_satisfied().unwrap()), src/prover.rs:193 ----
 * The reference checks the assignment in debug builds only; g16_prove, like a release build, proves whatever it is given, and for an
 * assignment that does not satisfy the constraints returns G16_OK and a well-formed proof that no verifier accepts.  The calls below
 * restate ark-relations' is_satisfied / which_is_unsatisfied over the matrices a g16_circuit already holds on the device: one more
 * gather-bound walk of A, B and C.  Row i < num_constraints fails when <A_i, z> * <B_i, z> != <C_i, z>; the
 * instance-copy rows the witness maps append are no constraints and are not looked at.
 * g16_check_result: n_unsatisfied rows fail, first_row is the lowest of them (what which_is_unsatisfied names) and a, b, c are its three
 * sums, Montgomery Fr like every scalar of this header; first_row = UINT64_MAX and a = b = c = 0 when no row fails. */
typedef struct {
    uint64_t n_unsatisfied;
    uint64_t first_row;
    uint64_t a[4], b[4], c[4];
} g16_check_result;
/* A Circom circuit holds A and B only (the map computes c = a .* b itself), so nothing on the device could notice that C z disagrees:
 * this uploads C (host view over num_constraints rows; the view carries no row count of its own, row_ptr is read as
 * num_constraints + 1 entries) and marks its unit coefficients like those of A and B.  The witness map still does not read C.  On a
 * Libsnark circuit, and on a circuit that already has C, nothing happens: G16_OK.  Not while another call is using the circuit.
 * G16_ERR_BAD_ARG: NULL, another curve or context, a row_ptr that does not start at 0, decreases or gives a row 2^32 terms, NULL col /
 * val with entries present, a column >= num_variables (g16_last_error says which). */
int g16_circuit_attach_c(g16_ctx* ctx, g16_circuit* circuit, const g16_csr_view* c);
/* is_satisfied / which_is_unsatisfied of (circuit, full_assignment).  G16_OK means the check RAN; the answer is in *out
 * (out->n_unsatisfied == 0: satisfied).  A host assignment is uploaded whole, in one copy, into a buffer the context keeps; a device
 * assignment is read in place.  num_constraints == 0 gives {0, UINT64_MAX}.  A multi-device context checks on its first device (the
 * circuit is replicated there; a device assignment must live on that device).
 * G16_ERR_BAD_LENGTH: n_assign != num_variables.  G16_ERR_BAD_ARG: NULL, another curve, a circuit of another GPU, a Circom circuit
 * without C (g16_circuit_attach_c first; g16_last_error says so), a Libsnark circuit with a row of 2^32 terms or more. */
int g16_circuit_check(g16_ctx* ctx, const g16_circuit* circuit, const uint64_t* full_assignment, uint64_t n_assign,
                      int assignment_on_device, g16_check_result* out);
/* g16_prove with the assertion of prover.rs:193 kept: arguments as g16_prove, plus check_out (may be NULL).  A host assignment is
 * uploaded once, checked, and proved from the resident copy through g16_prove(.., assignment_on_device = 1, ..) -- which gives up the
 * overlap of g16_prove's piecewise upload with the first mat-vec rows; a device assignment is checked in place.  (A multi-device
 * context checks on its first device and then proves from the caller's pointer as g16_prove does: every device stages its own copy.)
 * Unsatisfied: G16_ERR_UNSATISFIED, *out untouched, *check_out filled, no MSM launched.  Satisfied: whatever g16_prove returns for the
 * same inputs, the same proof bit for bit.  Errors of g16_circuit_check and of g16_prove as there. */
int g16_prove_checked(g16_ctx* ctx, const g16_pk* pk, const g16_circuit* circuit, const uint64_t* full_assignment,
                      uint64_t n_assign, int assignment_on_device, const uint64_t r[4], const uint64_t s[4], g16_proof* out,
                      g16_check_result* check_out);
/* CPU only: the same check by the same row walk compiled for the host, over the caller's own arrays (abc: A, B, C over num_constraints
 * rows; n_assign Fr).  G16_ERR_BAD_LENGTH for a malformed row_ptr or a column >= n_assign, G16_ERR_BAD_ARG for NULL or an unknown curve. */
int g16_host_circuit_check(int curve, const g16_csr_view abc[3], uint64_t num_constraints, const uint64_t* full_assignment,
                           uint64_t n_assign, g16_check_result* out);

/* sharded proof: every rank runs _partial on its pk shard, the host gathers the records, any rank
 * (all ranks, typically) runs _finalize over all of them */
int g16_prove_partial(g16_ctx* ctx, const g16_pk* pk, const g16_circuit* circuit, const uint64_t* full_assignment,
                      uint64_t n_assign, int assignment_on_device, int skip_b_g1, g16_partial* out);
int g16_prove_finalize(g16_ctx* ctx, const g16_pk* pk, const g16_partial* parts, int n_parts, const uint64_t r[4],
                       const uint64_t s[4], g16_proof* out);

/* Optional, before (or while) the ranks' g16_prove_partial calls run: start on a host thread the half of the glue of
 * src/prover.rs:76-131 that depends only on r, s and the key's fixed points -- r delta, s delta, r s delta and, by linearity of
 * :94 and :114, s (r delta_g1 + a_query[0] + alpha_g1) and r (s delta_g1 + b_g1_query[0] + beta_g1).  The next g16_prove_finalize on
 * this context over the same (pk, r, s) then only multiplies the two MSM sums by s and r, adds, and converts to affine; any other
 * (pk, r, s) ignores the prepared half.  g16_prove does this by itself. */
int g16_prove_finalize_prepare(g16_ctx* ctx, const g16_pk* pk, const uint64_t r[4], const uint64_t s[4]);

/* ---- distributed witness map (the Amdahl term of the sharded proof) ----
 * h = witness_map_from_matrices (src/r1cs_to_qap.rs:172-235) over `world` ranks (a power of two <= 16 with world^2 | domain_size),
 * every n-point transform as a local (n / world)-point transform, a twiddle, ONE all-to-all and a local world-point transform.
 * Rank r ends with the h coefficients of its BLOCK indices  (r * blk + j) + M * k1,  j < blk = M / world, k1 < world, M = n / world,
 * in the order [k1][j] -- which is how that rank's h_query shard has to be gathered (g16_pk_view.h = those bases, start 0).
 * The caller owns the buffers (device memory, M = g16_dwm_local_size() Fr each) and the exchange: after stages 0, 1 (three
 * arrays: a, b, c) and 2 (one array), chunk p (M / world elements) of each work array goes to rank p, which stores the chunk
 * from rank q at position q of the matching recv array -- an all-to-all (RCCL over xGMI: torch.distributed.all_to_all_single).
 *   stage 0: full_assignment -> work[0..2]     stage 1: recv[0..2] -> work[0..2]     stage 2: recv[0..2] -> work[0]
 *   stage 3: recv[0] -> h_local.               Each call returns with its device work finished. */
typedef struct g16_dwm g16_dwm;
int g16_dwm_create(g16_ctx* ctx, const g16_circuit* circuit, int rank, int world, g16_dwm** out);
void g16_dwm_free(g16_dwm* d);
uint64_t g16_dwm_local_size(const g16_dwm* d);
int g16_dwm_stage(g16_ctx* ctx, g16_dwm* d, int stage, const uint64_t* full_assignment, uint64_t n_assign, int assignment_on_device,
                  uint64_t* const work[3], uint64_t* const recv[3], uint64_t* h_local);
/* The same stages WITHOUT host synchronisation: the stage is enqueued on the context's witness-map stream (g16_ctx_wm_stream) and the
 * call returns; the caller enqueues its exchange on that SAME stream (e.g. torch.cuda.ExternalStream), so stages and exchanges are
 * ordered by the stream alone.  full_assignment must be device memory.  A following g16_prove_partial_h orders its h sort and its
 * bucket passes after everything enqueued on that stream; its witness digit/sort pass (shared by the MSMs of prover.rs:74,92,105,
 * 113) does not wait and runs beside the map's stages and exchanges. */
void* g16_ctx_wm_stream(g16_ctx* ctx);
int g16_dwm_stage_async(g16_ctx* ctx, g16_dwm* d, int stage, const uint64_t* full_assignment_dev, uint64_t n_assign,
                        uint64_t* const work[3], uint64_t* const recv[3], uint64_t* h_local);
/* Optional, before the stages above: enqueue NOW the witness digit/sort pass (shared by the MSMs of prover.rs:74,92,105,113) that the
 * next g16_prove_partial / g16_prove_partial_h over the same (pk shard, device assignment) would otherwise enqueue after the map's
 * forty launches -- so that sort and map run side by side from the start.  The next such call consumes it; any other call on the
 * context drops it (the sort's buffers live in the per-call arena). */
int g16_prove_partial_prepare(g16_ctx* ctx, const g16_pk* pk, const g16_circuit* circuit, const uint64_t* full_assignment_dev,
                              uint64_t n_assign);
/* g16_prove_partial with h supplied by the caller (device memory, h_len Fr; the key's h shard indexes it from h.start) */
int g16_prove_partial_h(g16_ctx* ctx, const g16_pk* pk, const g16_circuit* circuit, const uint64_t* full_assignment, uint64_t n_assign,
                        int assignment_on_device, const uint64_t* h_dev, uint64_t h_len, int skip_b_g1, g16_partial* out);

/* the same fold + glue without a GPU context: only the eight fixed points of `fixed` are read.  Lets a host
 * process that merely aggregates shard records (or the CPU multi-rank tests) finish a proof. */
int g16_finalize_host(int curve, const g16_pk_view* fixed, const g16_partial* parts, int n_parts, const uint64_t r[4],
                      const uint64_t s[4], g16_proof* out);

int g16_get_timings(g16_ctx* ctx, g16_timings* out);

/* diagnostics behind bench.py's `roofline.valu_bound` (no reference counterpart): the issue rate of v_mad_u64_u32 -- the
 * instruction the field products are made of -- measured on this GPU now (all CUs, 8 waves per SIMD, independent chains), and
 * the multiply-adds one mixed addition of the G1 / G2 bucket kernels executes, counted from the same constexpr tables the
 * kernels are generated from (limb count, relaxed columns) */
typedef struct {
    double mad_per_s;          /* measured: v_mad_u64_u32 lane-operations per second, whole GPU                  */
    double mads_per_add_g1;    /* static: multiply-adds per G1 mixed addition (8 products + 2 squarings)           */
    double mads_per_add_g2;    /* static: per G2 mixed addition, both lanes of the pair together                   */
    double mads_per_product;   /* static: one base-field product (limb products + Montgomery reduction + relaxation) */
    int limbs;                 /* 30-bit limbs of the base field                                                   */
} g16_diag;
int g16_diag_valu(g16_ctx* ctx, g16_diag* out);

/* ---- unit-level entry points (parity tests, micro-benchmarks) ---- */

/* h_out: domain_size Fr, natural order.  Leaves g16_timings.witness_map_ms / ntt_ms of this call behind (HIP events around the map
 * alone: neither the staging of a host assignment nor the download of h_out, which the call's wall time includes) */
int g16_witness_map(g16_ctx* ctx, const g16_circuit* circuit, const uint64_t* full_assignment, uint64_t n_assign,
                    int on_device, uint64_t* h_out);
/* bases affine, scalars Fr in Montgomery form (into_bigint is applied on the GPU, prover.rs:63-65);
 * out: affine result */
int g16_msm_g1(g16_ctx* ctx, const uint64_t* bases, const uint64_t* scalars, uint64_t n, uint64_t* out_affine);
int g16_msm_g2(g16_ctx* ctx, const uint64_t* bases, const uint64_t* scalars, uint64_t n, uint64_t* out_affine);
/* rank's bucket-space share of the same MSM (g16_pk_load_bucket_shard's cut, window tables built on the fly): the `world`
 * results add up to g16_msm_g1 / _g2 of the same inputs.  Parity tests. */
int g16_msm_bucket_shard(g16_ctx* ctx, int g2, const uint64_t* bases, const uint64_t* scalars, uint64_t n, int rank, int world,
                         uint64_t* out_affine);
/* in place, natural order in and out, n = 2^log_n Fr in host memory */
int g16_ntt(g16_ctx* ctx, uint64_t* data, int log_n, int inverse, int coset);

/* ---- synthetic workload generators (bench.py) ---- */

/* n distinct non-identity points P_i = (s0 + first + i) * G written to DEVICE memory `out_dev`
 * (g2 = 0: G1 affine, 1: G2 affine) */
int g16_synth_bases(g16_ctx* ctx, int g2, uint64_t seed, uint64_t first, uint64_t n, uint64_t* out_dev);
/* SYN(k, seed) Fibonacci-product-chain R1CS: n_c = 2^k - 2, 2 instance variables, 2^k + 1 variables.
 * Host buffers: z_out (2^k+1) Fr, row_ptr n_c+1, colA/B/C n_c each, val n_c Fr (all one, shared). */
int g16_synth_circuit(int curve, int k, uint64_t seed, uint64_t* z_out, uint64_t* row_ptr, uint32_t* colA,
                      uint32_t* colB, uint32_t* colC, uint64_t* val);

/* ---- CRS generation: Groth16::generate_parameters_with_qap, src/generator.rs:47-208 ----
 * The matrices-level form, like g16_prove: the caller synthesises the circuit (generator.rs:62-76) and passes
 * cs.to_matrices().  The reference draws t from the rng (generator.rs:90); here it comes with the rest of the toxic
 * waste so that a run can be replayed.  Scalar work (Lagrange coefficients at t, a/b/c(t), l, gamma_abc, h scalars:
 * r1cs_to_qap.rs:120-170, 236-246) runs on the host, the ~5n fixed-base multiplications on the GPU. */
typedef struct {
    uint64_t alpha[4], beta[4], gamma[4], delta[4], t[4]; /* Fr, arkworks Montgomery limbs */
} g16_toxic_waste;

#define G16_PARAMS_DEVICE_PTRS 1u /* the five query arrays below are device memory of the ctx's GPU */

typedef struct {
    uint64_t *alpha_g1, *beta_g1, *delta_g1; /* one G1 affine each, host memory                                   */
    uint64_t *beta_g2, *delta_g2, *gamma_g2; /* one G2 affine each, host memory                                   */
    uint64_t* gamma_abc_g1;                  /* num_inputs G1, host memory (VerifyingKey, data_structures.rs:39)  */
    uint64_t *a_query, *b_g1_query;          /* num_variables G1 each; entry 0 belongs to the constant-one variable */
    uint64_t* b_g2_query;                    /* num_variables G2                                                  */
    uint64_t* h_query;                       /* g16_h_query_len(qap, domain_size) G1: domain_size - 1 (Libsnark)   */
    uint64_t* l_query;                       /* num_variables - num_inputs G1                                     */
    uint32_t flags;
} g16_params_view;

/* status: G16_ERR_DEGREE_TOO_LARGE as in the prover; G16_ERR_UNEXPECTED_IDENTITY for gamma == 0 or delta == 0;
 * G16_ERR_BAD_ARG if t lies in the evaluation domain (sample_element_outside_domain never returns such a t) */
int g16_generate_parameters(g16_ctx* ctx, const g16_csr_view abc[3], uint64_t num_inputs, uint64_t num_constraints,
                            uint64_t num_variables, const g16_toxic_waste* toxic_waste, const uint64_t* g1_generator,
                            const uint64_t* g2_generator, const g16_params_view* out);
/* The same with the reduction chosen (g16_qap): g16_generate_parameters is this with qap = 0.  Circom: h_query has domain_size
 * entries (QAP::h_query_scalars, generator.rs:168), abc[2] is still read (gamma_abc / l need C(t)); G16_ERR_BAD_ARG also if
 * t = rho^j for an odd j, where the h scalars' closed form is undefined. */
int g16_generate_parameters_qap(g16_ctx* ctx, const g16_csr_view abc[3], uint64_t num_inputs, uint64_t num_constraints,
                                uint64_t num_variables, int qap, const g16_toxic_waste* toxic_waste,
                                const uint64_t* g1_generator, const uint64_t* g2_generator, const g16_params_view* out);
/* entries of h_query: domain_size - 1 (Libsnark), domain_size (Circom); 0 for an unknown qap or domain_size == 0 */
uint64_t g16_h_query_len(int qap, uint64_t domain_size);
/* CPU only, the code the generator runs: QAP::h_query_scalars(domain_size - 1, t, zt, delta_inverse) -- g16_h_query_len Fr out.
 * Libsnark: zt delta^-1 t^i with zt = t^n - 1 computed here.  G16_ERR_BAD_ARG: unknown qap, domain_size no power of two, Circom
 * with t = rho^j for an odd j; G16_ERR_DEGREE_TOO_LARGE as the generator. */
int g16_host_h_query_scalars(int curve, int qap, uint64_t domain_size, const uint64_t t[4], const uint64_t delta_inverse[4],
                             uint64_t* out);
/* CPU only: LibsnarkReduction::instance_map_with_evaluation (r1cs_to_qap.rs:120-170) -- a, b, c: num_variables Fr each */
int g16_host_qap_evaluations(int curve, const g16_csr_view abc[3], uint64_t num_inputs, uint64_t num_constraints,
                             uint64_t num_variables, const uint64_t t[4], uint64_t* a_out, uint64_t* b_out,
                             uint64_t* c_out, uint64_t zt_out[4]);

/* ---- setup from an SRS: a proving key nobody holds the toxic waste of ----
 * The calls above take alpha, beta, gamma, delta and t as scalars: fine for benchmarks and parity tests, useless for a deployed
 * verifier.  Here the key is derived from a phase-1 SRS (powers of tau) by group operations alone, then each party multiplies its
 * delta in.  With n = the power of two >= num_constraints + num_inputs:
 *   g16_generate_parameters_srs   the Lagrange-basis points [L_i(tau)] G as inverse n-point transforms over the group, the queries as
 *                                 sparse products over those points, h_query from tau_g1[n ..] -- gamma = delta = 1;
 *   g16_params_apply_delta        delta_g1, delta_g2 <- delta (.), every l_query / h_query point <- delta^-1 (.).
 * A key made this way and given ONE delta equals g16_generate_parameters_qap(alpha, beta, gamma = 1, delta, t = tau) byte for byte.
 * Whether an SRS is well formed and a contribution honest is tested by the companion library libg16_ceremony.so (g16_ceremony.h).
 * Phase 1 itself -- contributing to a powers-of-tau SRS and checking such a contribution -- is libg16_phase1.so (g16_phase1.h).
 * Not covered: .ptau / .zkey files, proofs of knowledge and the transcript, gamma != 1. */
typedef struct {
    uint64_t* tau_g1;       /* tau^i G1, i < n_tau_g1: G1 affine, Montgomery limbs, host memory (as g16_params_view) */
    uint64_t n_tau_g1;      /* needs >= 2n - 1                                                                     */
    uint64_t* tau_g2;       /* tau^i G2, i < n_tau_g2                                                              */
    uint64_t n_tau_g2;      /* needs >= n                                                                          */
    uint64_t* alpha_tau_g1; /* alpha tau^i G1, i < n_alpha_beta                                                    */
    uint64_t* beta_tau_g1;  /* beta tau^i G1, i < n_alpha_beta                                                     */
    uint64_t n_alpha_beta;  /* needs >= n                                                                          */
    uint64_t* beta_g2;      /* beta G2, one point                                                                  */
} g16_srs_view;

/* entries one lane of the sparse products walks at most: longer columns (the constant-one wire) are cut into segments of this
 * length, one lane each, and the segment sums are folded the same way, level by level */
#define G16_SRS_SEGMENT_LEN 32
uint64_t g16_srs_segment_len(void);

/* Stands in for evaluate_all_lagrange_coefficients + the batch multiplications of generator.rs:129-183 and for
 * instance_map_with_evaluation / h_query_scalars (r1cs_to_qap.rs:120-170, 236-246), with points for scalars.  Arguments and matrix
 * validation as g16_generate_parameters_qap (a multi-device context runs on its first device).  An SRS longer than needed is
 * accepted and its prefix used; one too short gives G16_ERR_BAD_LENGTH with g16_last_error naming the array.  `out` as in
 * g16_generate_parameters_qap, host memory only: G16_PARAMS_DEVICE_PTRS is refused with G16_ERR_BAD_ARG.
 * out->gamma_g2 = out->delta_g2 = tau_g2[0], out->delta_g1 = tau_g1[0]. */
int g16_generate_parameters_srs(g16_ctx* ctx, const g16_csr_view abc[3], uint64_t num_inputs, uint64_t num_constraints,
                                uint64_t num_variables, int qap, const g16_srs_view* srs, const g16_params_view* out);
/* In place over delta_g1, delta_g2 and the first n_l_query / n_h_query points of l_query / h_query (host memory; the other fields
 * of `inout` are not read).  G16_ERR_UNEXPECTED_IDENTITY for delta == 0 (generator.rs:110-111). */
int g16_params_apply_delta(g16_ctx* ctx, const uint64_t delta[4], const g16_params_view* inout, uint64_t n_l_query,
                           uint64_t n_h_query);
/* The transform of step 1 on its own, as g16_ntt is for the scalar transforms: out[i] = sum_k w^(ik) points[k] over n = 2^log_n
 * affine points (g2 = 0: G1, 1: G2), or with w^-1 and the factor n^-1 when `inverse`.  Natural order in and out, host memory;
 * `out` may alias `points`. */
int g16_group_ntt(g16_ctx* ctx, int g2, const uint64_t* points, int log_n, int inverse, uint64_t* out);
/* A TEST AND BENCHMARK UTILITY: an SRS from known secrets (a real one comes from a ceremony whose secrets are gone), built with
 * the fixed-base kernels of g16_generate_parameters.  Fills n_tau_g1 points of out->tau_g1, n_other points of tau_g2,
 * alpha_tau_g1 and beta_tau_g1, and beta_g2; the counts in `out` say what the buffers hold and must not be smaller. */
int g16_srs_from_trapdoor(g16_ctx* ctx, const uint64_t tau[4], const uint64_t alpha[4], const uint64_t beta[4],
                          const uint64_t* g1_generator, const uint64_t* g2_generator, uint64_t n_tau_g1, uint64_t n_other,
                          const g16_srs_view* out);
/* stream-event times of the last g16_generate_parameters_srs (transforms, sparse products, h step) and g16_params_apply_delta
 * (delta step) on this context, in milliseconds */
typedef struct {
    double transforms_ms, products_ms, h_ms, delta_ms;
} g16_srs_timings;
int g16_srs_get_timings(g16_ctx* ctx, g16_srs_timings* out);
/* CPU only: the same butterflies and the same sums in plain host code over the same group arithmetic (the `not gpu` tests) */
int g16_host_group_ntt(int curve, int g2, const uint64_t* points, int log_n, int inverse, uint64_t* out);
int g16_host_generate_parameters_srs(int curve, const g16_csr_view abc[3], uint64_t num_inputs, uint64_t num_constraints,
                                     uint64_t num_variables, int qap, const g16_srs_view* srs, const g16_params_view* out);

/* ---- canonical (de)serialisation of points (CPU) ----
 * The element format behind `#[derive(CanonicalSerialize, CanonicalDeserialize)]` on Proof / VerifyingKey / ProvingKey
 * (src/data_structures.rs:8,31,125): BLS12-381 in the zcash / IETF form that ark-bls12-381 uses, BN254 in ark-ec's
 * default short-Weierstrass form (see serialize.hip; restated from the published formats, not checkable against the
 * reference here).  Containers (Vec<T> = u64 little-endian length + elements, struct = fields in order) are assembled by the
 * caller (groth16_amd/serialize.py).  `points`: affine Montgomery limbs as everywhere in this ABI. */
uint64_t g16_serialized_point_size(int curve, int g2, int compressed);
int g16_serialize_points(int curve, int g2, int compressed, const uint64_t* points, uint64_t n, uint8_t* out);
/* validate: 0 = Validate::No, 1 = on-curve check, 2 = on-curve + prime-order subgroup (Validate::Yes).
 * G16_ERR_INVALID_DATA for a non-canonical coordinate, inconsistent flags, an x with no point, or a failed check */
int g16_deserialize_points(int curve, int g2, int compressed, const uint8_t* in, uint64_t n, int validate,
                           uint64_t* points_out);

/* ---- host-side arithmetic self-test hooks (CPU; used by the `not gpu` tests) ----
 * The same field / group code the kernels use, compiled for the host -- with one exception: the Montgomery product.  On the host
 * Fp::operator* runs a 64-bit-limb body (Fp::mul_host64), on the device the 32-bit operand-scanning body (Fp::mul_cios32); +, -,
 * to_canonical and the group formulas are one text for both.  These hooks therefore run the host's product; the device's is tested
 * by the standard-form lab below (g16_host_std_op forms 14 / 15 / 18 on the CPU, g16_dev_std_op on the GPU).
 * They ship IN the product library on purpose: the CPU tier --
 * the only tier that runs where the library is built, a container without a GPU -- checks the 30-bit lazy arithmetic, its overflow
 * and bound proofs, the window-table tasks and the bucket-method model (g16_host_selftest, g16_host_msm_model[_shard]) on exactly the
 * code objects the kernels are generated from.  None of them is on a proof's path; none touches a GPU.
 * which: 0 Fr, 1 Fq.  op: 0 add, 1 sub, 2 mul, 3 inverse(a), 4 to_canonical(a), 5 from_canonical(a) */
int g16_host_field_op(int curve, int which, int op, const uint64_t* a, const uint64_t* b, uint64_t* out);
/* g2: 0/1.  op: 0 p+q (affine in, affine out), 1 k*p (k canonical 4 limbs), 2 p+q via XYZZ+XYZZ add */
int g16_host_group_op(int curve, int g2, int op, const uint64_t* p, const uint64_t* q_or_k, uint64_t* out);
/* CPU model of the MSM bucket method exactly as the kernels run it (signed digits, window c):
 * checks digit extraction + bucket reduction + window fold logic without a GPU */
int g16_host_msm_model(int curve, int g2, const uint64_t* bases, const uint64_t* scalars, uint64_t n, int c,
                       uint64_t* out_affine);
/* the same model of rank's bucket-space share (c < 0: merged plan with window size -c) */
int g16_host_msm_model_shard(int curve, int g2, const uint64_t* bases, const uint64_t* scalars, uint64_t n, int c, int rank,
                             int world, uint64_t* out_affine);

/* randomized CPU self-test of the reduced-radix (30-bit limb) arithmetic used by the bucket kernel against the
 * standard field / group code; 0 = all checks passed, otherwise the number of the first failing check */
int g16_host_selftest(int curve, uint64_t seed, int iters);

/* ---- the field lab (test hooks): ONE operation of the kernels' 30-bit-limb field arithmetic on raw limbs ----
 * g16_dev_fp30_op runs one tuple per lane on the ctx's (first) GPU -- the product forms through the generated assembly blocks, the
 * lane-pair forms with one Fq2 value per adjacent lane pair -- and g16_host_fp30_op runs the same code compiled for the host.
 * field: 0 Fr, 1 Fq of the curve.  A slot is NL 32-bit words (NL = 13 for BLS12-381's Fq, 9 for the other three fields): 30-bit limbs,
 * or the packed / standard form's 32-bit words padded with zeros, or a flag / small integer in word 0.  operands: n tuples of `in`
 * slots; out: n tuples of `out` slots.  Preconditions are those of fp30.hpp; nothing is checked.  form (in -> out slots):
 *   0 mul (2->1)  1 sqr (1)  2 mul2 = x0 y0 + x1 y1 (4)  3 mul4 (8)  4 / 6 / 8 mul_s2 / _s4 / _s8 = x y + K p - s (3)
 *   5 / 7 / 9 mul2_s2 / _s4 / _s8 (5)  10 mul_x3 = x y + 6 p - (u + 2 v) (4)  11 sqr_x3 (3)                      [4..11: Fq only]
 *   20..24 sub<K> = a + K p - b for K = 2, 4, 6, 8, 16 (2)  25 add_dbl = a + 2 b (2)  26 normalize (1)
 *   27 sub_pow2(a, b, k) = a + 2^(k+1) p - b, k in word 0 of the third slot (3; Fr only)
 *   28 unpack_cond_neg(packed y, flip) and cond_neg2(unpack(y), flip) (2->2)
 *   30..33 cond_sub<K> for K = 2, 4, 8, 16  34 weak_reduce32  35 canonical_lt2p  36 canonical_lt8p  37 canonical_quick
 *   38 neg_canonical  39 maybe_zero (flag)  40 is_zero_exact (flag)  41 to_std (words out)  42 std_to_r30 (words in and out)
 *   43 to_packed (words out)                                                                                       [30..43: 1->1]
 *   50 Fp2x30 mul (a0 a1 b0 b1 -> c0 c1)  51 Fp2x30 sqr (2->2)                                                      [Fq only]
 *   lane pair (Fq only; Fq2 operand k in slots 2 k, 2 k + 1; 2 slots out): 60 mul_v(lhs a, rhs b)  61 sqr_v(lhs a)
 *   62 sqr_sub_x3_v(lhs a, u, v)  63 mul_add_fused(a, b, c, d)  64 mul_sub_fused(a, b, c, d) (pair_mul_sub)
 *   65 mul_add_fused_v(lhs a, rhs b, lhs c, rhs d)
 *   accumulator (Fq only): a lazy XYZZ accumulator (Acc30) takes up to three mixed additions.  70 G1 (11 -> 5 slots), 71 G2 one lane,
 *   72 G2 lane pair (21 -> 9; device only).  A field element takes C slots (1 for Fq, 2 for Fq2).  in: x y zz zzz raw lazy limbs |
 *   a flag slot: word 0 the accumulator is the identity, word 1 the number of points, word 2 + j point j is the identity | x y of
 *   three affine points (limbs, below 2 p).  out: x y zz zzz canonical in the packed form's words | word 0: the result is the identity
 *   parked accumulator (Fq only): the bucket pass's own form -- AccParked, coordinates parked in LDS in the kernel's layout, signed
 *   additions from packed y, the flush's gather().  73 parked_chain_g1 (11 -> 5 slots; the host twin parks in plain memory),
 *   74 parked_chain_g2_pair (lane pair, 21 -> 9; device only).  in: x y zz zzz raw lazy limbs AS PARKED (the sum is their negative
 *   when neg is set) | a flag slot: word 0 the accumulator is the identity, word 1 the initial neg, word 2 the number of points,
 *   word 3 + j point j is the identity, word 6 + j point j is subtracted | x y of three affine points (canonical, the packed form's
 *   words).  out: as 70..72
 *   inversion and the window-table / batched-affine arithmetic (Fq only; batch_affine.hpp, window_tables.hpp):
 *   80 inv_plain = ModInv30::inverse_plain (1->1): normalised limbs of any value below 2^(30 NL - 3) -> canonical limbs of x^-1 mod p
 *      as a plain integer, 0 when p divides x  81 inv = batch_inverse(Fp30) (1->1): same operands, residue x^-1 R'^2, below 1.5 p
 *   82 pair_inv = batch_inverse(Fp2p30) on the lane pair (c0 c1 -> c0 c1; the host twin calls pair_inverse with hi = false and true):
 *      components below 16 p in (the callers stay below 1.5 p; a pair's own denominator reaches 3 p), below 1.5 p out,
 *      (c0 + c1 u) * out = R'^2, zero gives zero
 *   83 jac_dbl_g1 (4->3), 84 jac_dbl_g2_pair (lane pair, 7->6; device only): X Y Z raw lazy limbs (X < 5.8 p, Y < 5.5 p, Z < 3 p per
 *      component) | word 0 of the last slot: d, 1 <= d <= 32 (clamped) -> X Y Z after d times jac30_double
 *   85 aff_pair_g1 (5->3), 86 aff_pair_g2_pair (lane pair, 9->5; device only): one pair of the batched-affine tree --
 *      AffineBatch::classify, batch_inverse of its denominator, AffineBatch::finish.  in: a flag slot (word 0: P is the identity,
 *      word 1: Q is) | px py qx qy canonical limbs.  out: rx ry canonical limbs | word 0: the sum is the identity, word 1: the kind
 *      (0 ADD, 1 DBL, 2 TAKE_P, 3 TAKE_Q, 4 ZERO)
 * G16_ERR_BAD_ARG for an unknown form or one the field does not have, n == 0 or n > 2^22. */
int g16_dev_fp30_op(g16_ctx* ctx, int field, int form, const uint32_t* operands, uint64_t n, uint32_t* out);
int g16_host_fp30_op(int curve, int field, int form, const uint32_t* operands, uint64_t n, uint32_t* out);

/* ---- the table lab (test hook): the window-table builder in place ----
 * Uploads n affine points (the ABI's form: Montgomery limbs, all-zero = the identity; G2 when g2 != 0), calls the key loader's
 * build_window_tables for window size c and W rows -- its chunk loop, the parking buffer it allocates, its launch shape -- and
 * downloads the W * n records: table_out[j * n + i] = 2^(c j) P_i as the bucket pass reads it, x then y (G2: x.c0 x.c1 y.c0 y.c1),
 * each the canonical value times R' = 2^(30 NL) mod p in the packed form's words; an identity row is all zero.  The points are not
 * checked (not even for being on the curve: the doubling formulas never read b).  1 <= c <= 32, 1 <= W <= 64, n <= 2^18 + 4096 (just
 * past the builder's chunk of 2^18 points; W * n records of device memory, 3.3 GB at the limits for G2 on BLS12-381), else G16_ERR_BAD_ARG; W > 32 is the builder's own refusal, G16_ERR_INTERNAL; n == 0 returns G16_OK and writes nothing. */
int g16_dev_window_table_lab(g16_ctx* ctx, int g2, const uint64_t* points, uint64_t n, int c, int W, uint64_t* table_out);

/* ---- the tower lab (test hooks): ONE operation of the pairing tower (csrc/pairing.hpp) on raw limbs ----
 * g16_dev_pairing_op runs one tuple per lane on the ctx's (first) GPU and its curve, g16_host_pairing_op the same code compiled for
 * the host.  A slot is NL 32-bit words of the curve's Fq (13 for BLS12-381, 9 for BN254).  An Fq operand is RAW 30-bit limbs in the
 * R' Montgomery radix, ANY representative below 2 p (loaded straight into Q30::a); an Fq result is the raw limbs the operation left,
 * not canonicalised.  Fq2 is 2 slots (c0 c1), Fq6 is 6, Fq12 is 12, in arkworks' order c0.c0.c0 ... c1.c2.c1.  A flag, a small
 * integer or an exponent sits in the low words of a slot; "words" is the standard (arkworks) Montgomery form's 32-bit words padded
 * with zeros.  operands: n tuples of `in` slots; out: n tuples of `out` slots.  form (in -> out slots):
 *   Q30   0 a + b (2->1)  1 a - b  2 neg (1)  3 dbl (1)  4 a * b (2)  5 sqr (1)  6 is_zero (1 -> flag)  7 a == b (2 -> flag)
 *         8 inverse (1; of a zero residue: 0)  9 from_std then to_std (words -> words)
 *   T2    10 a + b (4->2)  11 a - b  12 neg (2->2)  13 conj  14 dbl  15 scale(a, k) (3->2)  16 mul_outlined (4->2)
 *         17 sqr_outlined (2)  18 inverse (2; of zero: zero)  19 mul_by_xi (2)  20 a == b (4 -> flag)
 *   T6    30 a + b (12->6)  31 a - b  32 neg (6->6)  33 mul_outlined (12->6)  34 mul_by_v (6)  35 inverse (6; of zero: zero)
 *   T12   40 mul_outlined (24->12)  41 sqr_outlined (12->12)  42 cyc_sqr_outlined  43 conj  44 inverse (of zero: zero)
 *         45 is_zero (12 -> flag)
 *   Pairing   50 frob(a, j): a | j = 1, 2, 3 in word 0 (13->12)  51 equal(a, b) (24 -> flag)  52 store_gt (12 -> 12 words)
 *         53 load_gt then store_gt (12 words -> 12 words)  54 ell(f, coeffs, P): f | c0 c1 c2 (Fq2 each) | P.x P.y (20->12)
 *         55 Proj::dbl_step: T = x y z (6 -> T' and c0 c1 c2: 12)  56 Proj::add_step: T | the affine addend x y (10->12)
 *         57 frob_twist(q, k): q.x q.y | k = 1, 2 in word 0 (5->4)  58 cyc_pow: a | the exponent's low and high word, > 0 (13->12)
 *         59 cyc_pow_bits: a | words 0..7 the exponent, word 8 the bit count <= 256 (13->12)  60 exp_by_x (12->12)
 *         61 final_exp (12 -> 12 and a flag slot: the returned bool; the value is zero where it is false)
 *         62 g1_on_curve: x y words (2 -> flag)  63 g2_on_curve: x.c0 x.c1 y.c0 y.c1 words (4 -> flag)
 * Preconditions are those of pairing.hpp (42, 58..60: a in the cyclotomic subgroup); nothing is checked.
 * G16_ERR_BAD_ARG for an unknown form, a null pointer, n == 0 or n > 2^22. */
int g16_dev_pairing_op(g16_ctx* ctx, int form, const uint32_t* operands, uint64_t n, uint32_t* out);
int g16_host_pairing_op(int curve, int form, const uint32_t* operands, uint64_t n, uint32_t* out);

/* ---- the standard-form lab (test hooks): ONE operation of csrc/field.hpp and csrc/curve.hpp on the ABI's own words ----
 * g16_dev_std_op runs one tuple per lane, in workgroups of 64, on the ctx's (first) GPU and its curve, g16_host_std_op the same code
 * compiled for the host.  kind: 0 Fr, 1 Fq, 2 Fq2, 3 G1, 4 G2.  A slot is one base-field element in the ABI's form: the Fp<P>'s 32-bit
 * words (8 for Fr and for BN254's Fq, 12 for BLS12-381's Fq), Montgomery, canonical (below p); Fq2 is 2 slots (c0 c1).  operands: n
 * tuples of `in` slots; out: n tuples of `out` slots.  form (in -> out slots):
 *   Fp    0 a + b (2->1)  1 a - b  2 neg (1)  3 dbl (1)  4 a * b through operator* (2; out of line for BLS12-381's Fq)  5 sqr (1)
 *         6 inverse (1; of zero: zero)  7 to_canonical (1 -> plain words)  8 from_canonical (plain words below p -> 1)
 *         9 flags (a b -> word 0 is_zero(a), word 1 is_one(a), word 2 a == b)
 *         14 a * b, 15 sqr, 18 from_canonical through Fp::mul_cios32 BY NAME: the device's 32-bit product on the host too.  On the
 *         device 4 / 5 / 8 run that body as well; on the host they run the 64-bit body (mul_host64) the host glue runs per proof
 *   Fp2   0 a + b (4->2)  1 a - b  2 neg (2)  3 dbl (2)  4 a * b (Karatsuba; 4->2)  5 sqr (complex squaring; 2)  6 inverse (2; of zero: zero)
 *   group (C = 1 slot per coordinate for G1, 2 for G2; an affine point is x y, the identity all zero; a raw XYZZ record is x y zz zzz,
 *         the identity any record with zz = 0)
 *         0 from_affine(P) then add_affine(Q) (4 C -> 4 C)  1 add of two raw records (8 C -> 4 C)  2 dbl of a raw record (4 C)
 *         3 dbl_affine (2 C -> 4 C)  4 neg of a raw record (4 C)  5 mul_bits: a raw record | words 0..7 of a slot the scalar | word 0 of
 *         a slot the bit count, <= 256 (clamped) (4 C + 2 -> 4 C)  6 to_affine of a raw record (4 C -> 2 C)
 *         XYZZ results come back raw (x y zz zzz as the formula left them), not normalised.
 * Nothing is checked about the operands.  G16_ERR_BAD_ARG for an unknown kind or form, a null pointer, n == 0 or n > 2^22. */
int g16_dev_std_op(g16_ctx* ctx, int kind, int form, const uint32_t* operands, uint64_t n, uint32_t* out);
int g16_host_std_op(int curve, int kind, int form, const uint32_t* operands, uint64_t n, uint32_t* out);

/* ---- the reduction lab (test hook): the MSM reductions alone, on caller-made partial sums ----
 * Fills a plan (merged: 0 per-window fold, 1 merged fold; `groups` groups of 2^(c-1) buckets, 2 <= c <= 16; G = 8, 16 or 32 buckets
 * per lane of the bucket reduction), the partial-sum slot offsets and the heavy-bucket list from nparts[groups * 2^(c-1)] (partial sums
 * per bucket), uploads `records` -- n_records = sum of nparts records in bucket order, each x y zz zzz as raw lazy 30-bit limbs (NL words
 * per Fq component: 4 NL words for G1, x.c0 x.c1 y.c0 ... 8 NL words for G2; the identity is an all-zero zz) -- and runs the prover's
 * reduction (heavy combine, bucket combine, bucket reduction, window reduction) and the host fold.  Preconditions are those the bucket
 * pass guarantees (x < 7.5 p, y < 4 p, zz, zzz < 1.8 p per component); nothing is checked.  The suite runs c = 6 with two groups
 * and every G; other window sizes are accepted as make_msm_plan accepts them and are not exercised by a test.
 * first_slots: groups * 2^(c-1) records, every bucket's first slot after the combine stages (zeros for a bucket without partial sums);
 * out_affine: the folded sum  sum_w 2^(c w) sum_b (b + 1) S_(w,b)  (per-window)  or  sum_k (k + 1) S_k over the bucket key k (merged). */
int g16_dev_msm_reduce_lab(g16_ctx* ctx, int g2, int merged, int c, int groups, int G, const uint32_t* nparts, const uint32_t* records,
                           uint64_t n_records, uint32_t* first_slots, uint64_t* out_affine);
/* The batch form, G1 only (the prover batches no G2 reductions): n_jobs = 1 .. 4 jobs over ONE plan (merged, c, groups, G as above), job j
 * with its own nparts[j], records[j] (n_records[j] of them), slot offsets, heavy list and device buffers, and its own first_slots[j] and
 * out_affine[j].  The jobs are reduced by the launches a proof makes (blockIdx.y / .z of every reduction kernel = job):
 *   mode 0, together: msm_reduce_batch over all jobs, first stage (heavy combine, bucket combine) included -- a proof's last batch with
 *           h inside; early_mask is not looked at
 *   mode 1, early:    the jobs whose bit is set in early_mask have their first stage in ONE launch per kernel (msm_heavy_reduce_batch),
 *           every other job has it alone (msm_heavy_reduce), then msm_reduce_batch over all jobs with heavy_done set -- the single-GPU
 *           proof, whose l / a / b_g1 batch has its first stage underneath the h pass
 * The fold runs per job.  G16_ERR_BAD_ARG: n_jobs outside 1 .. 4, another mode, in mode 1 an early_mask that is 0 or has a bit at or
 * above n_jobs, a null pointer; G16_ERR_BAD_LENGTH: a job whose n_records is not the sum of its nparts. */
int g16_dev_msm_reduce_batch_lab(g16_ctx* ctx, int merged, int c, int groups, int G, int n_jobs, int mode, uint32_t early_mask,
                                 const uint32_t* const* nparts, const uint32_t* const* records, const uint64_t* n_records,
                                 uint32_t* const* first_slots, uint64_t* const* out_affine);

/* ---- the pass lab (test hook): the bucket pass's walk in place, on a caller-made sorted list ----
 * A plan as in the reduction lab (merged, 2 <= c <= 16, `groups` groups of 2^(c-1) buckets, M = groups * 2^(c-1) <= 2^12 buckets, G = 8,
 * 16 or 32) with segment length lseg (8 .. 4096), and 1 to 4 jobs that share it.  A job is a table of rows * base_count affine points in
 * the ABI's form (rows = 1 for a per-window plan; row j of a merged plan's table is what window tag j addresses), uploaded as given and
 * converted to the bucket pass's radix; `shift` and `base_count` as msm_bucket_pass takes them; counts[M], the entries per bucket; and
 * `sorted`, the n_sorted = sum of counts entry words in bucket order, point | sign << 31 (merged: point | window << 26 | sign << 31).
 * offsets, task_off and the heavy list are derived by the library's own layout code (the tail of sort_scalars); the partial-sum slots --
 * task_off[M] records and 8 guard records behind them -- are filled with the byte 0xA5; the passes of all jobs run as ONE launch; the
 * reductions and the fold then run per job.  Written per job: n_records = task_off[M]; records[0 .. n_records + 8) as the pass left them
 * (the layout of the reduction lab's records; record_cap >= ceil(n_sorted / lseg) + M + 8, else G16_ERR_BAD_LENGTH); offsets, task_off and
 * heavy, M + 1 words each (heavy[0] = count, then bucket ids in any order); out_affine, the folded sum as in the reduction lab.
 * G16_ERR_BAD_ARG for what would let the kernel read outside what was uploaded: sum of counts != n_sorted, a merged entry whose window
 * tag is >= rows, lseg outside 8 .. 4096, n_sorted > 2^16, M > 2^12, base_count > 2^16, |shift| > 2^40, n_jobs outside 1 .. 4, a null
 * pointer.  A point index outside [0, base_count) after `shift` is NOT refused: the kernel skips such an entry. */
typedef struct {
    const uint64_t* table;
    uint64_t base_count;
    int64_t shift;
    const uint32_t* counts;
    const uint32_t* sorted;
    uint64_t n_sorted;
    uint64_t record_cap;
    uint32_t* records;      /* out */
    uint64_t n_records;     /* out */
    uint32_t* offsets;      /* out */
    uint32_t* task_off;     /* out */
    uint32_t* heavy;        /* out */
    uint64_t* out_affine;   /* out */
} g16_pass_lab_job;
int g16_dev_msm_pass_lab(g16_ctx* ctx, int g2, int merged, int c, int groups, int G, int lseg, int rows, g16_pass_lab_job* jobs, int n_jobs);

/* ---- the parts lab (test hook): the bucket-part walk in place ----
 * The pass lab with the walk the prover's merged-window sorts use: a bucket of n entries is cut into ceil(n / lmax) parts, part p covers
 * the entries [p n / np, (p + 1) n / np) of the bucket (integer division), slot task_off[b] + p holds part p's sum, and a lane walks one
 * part -- the task list is ordered by length, longest first -- and stores its sum once.  Same arguments, same jobs, same outputs and
 * the same refusals as g16_dev_msm_pass_lab, with lmax (8 .. 4096) in place of lseg: task_off is the exclusive prefix of
 * ceil(counts / lmax), heavy lists the buckets with more than 16 parts, record_cap >= n_sorted / lmax + M + 8.
 * g16_host_msm_parts_lab is the host twin for G1: one job, the same layout rule and the same per-task walk (part_walk.hpp) compiled for
 * the host, tasks in slot order; it fills records (n_records of them, no guards: record_cap >= n_sorted / lmax + M), offsets, task_off,
 * heavy and out_affine, and reads the job through exactly sized copies, so that a sanitizer build sees an index out of range. */
int g16_dev_msm_parts_lab(g16_ctx* ctx, int g2, int merged, int c, int groups, int G, int lmax, int rows, g16_pass_lab_job* jobs, int n_jobs);
int g16_host_msm_parts_lab(int curve, int merged, int c, int groups, int lmax, int rows, g16_pass_lab_job* job);

/* ---- the sort lab (test hook): signed digits and the sort layout in place ----
 * Uploads n <= 2^16 scalars (Fr, Montgomery limbs) and calls sort_scalars as the prover does: merged_c = 0 for a per-window plan (window
 * size from the cost model or G16_MSM_WINDOW), 9 .. 20 for a merged plan, shard_n > 1 for rank shard_r's bucket-space share of a merged
 * plan; G16_MSM_SEGMENT and the other environment knobs apply.  Returns the plan, the bounds the buffers were sized by, and the layout:
 * offsets, task_off and heavy (M + 1 words each, M = groups * B; bucket_cap words available, else G16_ERR_BAD_LENGTH) and the first
 * n_sorted = offsets[M] words of the sorted list (sorted_cap words available).  G16_MSM_AFFINE_LEVELS > 0 (padded bucket regions) is
 * refused with G16_ERR_BAD_ARG. */
typedef struct {
    int32_t c, W, groups, merged;
    uint32_t B, Lmax, max_tasks, max_segments;
    uint32_t K[10];          /* the signed-digit bias, little-endian words */
    uint32_t n_sorted;
    uint32_t reserved;
} g16_sort_lab_info;
int g16_dev_msm_sort_lab(g16_ctx* ctx, const uint64_t* scalars, uint64_t n, int merged_c, int shard_n, int shard_r, g16_sort_lab_info* info,
                         uint32_t* offsets, uint32_t* task_off, uint32_t* heavy, uint64_t bucket_cap, uint32_t* sorted, uint64_t sorted_cap);

/* ---- verifier (src/verifier.rs:13-76, src/lib.rs:84-96) ------------------------------------------------------------
 * GT values cross as 12 Fq in arkworks' order c0.c0.c0, c0.c0.c1, ..., c1.c2.c1 (Fq12 = Fq6[w]/(w^2 - v), Fq6 = Fq2[v]/(v^3 - xi)),
 * Montgomery limbs as every other field element: byte-equal to PairingOutput.0.  Pairings are optimal ate with the exact final
 * exponentiation f^((q^12 - 1) / r); a pair with an identity point contributes 1. */
typedef struct {
    const uint64_t* alpha_g1;     /* G1 affine */
    const uint64_t* beta_g2;      /* G2 affine */
    const uint64_t* gamma_g2;
    const uint64_t* delta_g2;
    const uint64_t* gamma_abc_g1; /* n_gamma_abc G1 affine points */
    uint64_t n_gamma_abc;
} g16_vk_view;                    /* VerifyingKey, data_structures.rs:31-44 */
typedef struct g16_pvk g16_pvk;   /* PreparedVerifyingKey (data_structures.rs:56-66), resident on the ctx's device(s) */
/* e(alpha, beta), the line coefficients of -gamma and -delta and window tables of gamma_abc_g1[1..], computed on the GPU */
int g16_pvk_load(g16_ctx* ctx, const g16_vk_view* vk, g16_pvk** out);
void g16_pvk_free(g16_pvk* pvk);
int g16_pvk_alpha_beta(const g16_pvk* pvk, uint64_t* out_fq12);
/* proofs: n x (A | B | C) affine; public_inputs: n x num_public Fr.  verdicts[i]: 1 accept, 0 the pairing equation fails,
 * 2 A, B or C is not on its curve (a superset of the reference, whose point types cannot hold such points).
 * G16_ERR_MALFORMED_VK fails the whole call when num_public + 1 != n_gamma_abc.  A multi-device ctx cuts the batch into one
 * chunk per device; verdicts stay in input order.
 * An input is four words of Montgomery limbs and is NOT compared with r: every verifier call -- this one, the prepared-input lab,
 * the three aggregate calls, the mixed call and the g16_host_ forms -- reads words of any value m < 2^256 as the field element
 * m R^-1 mod r, so x and x + r are the same input (a caller that keys anything on the raw words canonicalises them). */
int g16_verify_batch(g16_ctx* ctx, const g16_pvk* pvk, const uint64_t* proofs, uint64_t n, const uint64_t* public_inputs,
                     uint64_t num_public, uint8_t* verdicts);
/* the same with IC = prepare_inputs(..) given per proof (n G1 affine) */
int g16_verify_batch_prepared(g16_ctx* ctx, const g16_pvk* pvk, const uint64_t* proofs, const uint64_t* prepared_inputs, uint64_t n,
                              uint8_t* verdicts);
/* prod_i e(g1s[i], g2s[i]) on the ctx's (first) GPU; G16_ERR_UNEXPECTED_IDENTITY if the Miller loop gave 0 (verifier.rs:62) */
int g16_pairing(g16_ctx* ctx, const uint64_t* g1s, const uint64_t* g2s, uint64_t n_pairs, uint64_t* out_fq12);
/* the same templates on the CPU (no GPU needed) */
int g16_host_pairing(int curve, const uint64_t* g1s, const uint64_t* g2s, uint64_t n_pairs, uint64_t* out_fq12);
int g16_host_verify(int curve, const g16_vk_view* vk, const uint64_t* proof, const uint64_t* public_inputs, uint64_t num_public,
                    uint8_t* verdict);
/* Randomised batch verification: ALL n proofs under one key in one equation with one final exponentiation,
 *   FE(prod_i ML(r_i A_i, B_i) * ML(sum_i r_i IC_i, -gamma) * ML(sum_i r_i C_i, -delta)) == e(alpha, beta)^(sum_i r_i).
 * *verdict: 1 every proof is accepted; 0 the equation fails (at least one proof is invalid; g16_verify_batch names it); 2 some
 * proof has a point off its curve (2 wins over 0).  n = 0 gives 1.
 * coeffs: n x 2 words, the little-endian 128-bit r_i; a zero coefficient is G16_ERR_BAD_ARG (its proof would drop out of the check).
 * Explicit coefficients make the call deterministic and let a caller supply transcript-derived values; they must be fixed AFTER the
 * proofs.  coeffs == NULL: the library draws them from the operating system's generator (getrandom(2)), redrawing a zero.
 * Contract: a batch with an invalid proof is accepted with probability about 2^-127 over the coefficients, PROVIDED the points of
 * every proof lie in the prime-order subgroups -- what the reference guarantees by deserialising with Validate::Yes and what
 * g16_deserialize_points with validation does here.  Like verify_proof itself, this function checks on-curve only;
 * g16_verify_aggregate_checked below runs the membership tests on the GPU first and needs no such proviso.
 * G16_ERR_MALFORMED_VK as g16_verify_batch.  A multi-device ctx cuts the batch into one chunk per device; the once-per-batch tail
 * (two prepared pairs, the final exponentiation, the GT power) runs on the calling host thread. */
int g16_verify_aggregate(g16_ctx* ctx, const g16_pvk* pvk, const uint64_t* proofs, uint64_t n, const uint64_t* public_inputs,
                         uint64_t num_public, const uint64_t* coeffs, uint8_t* verdict);
/* the same templates on the CPU */
int g16_host_verify_aggregate(int curve, const g16_vk_view* vk, const uint64_t* proofs, uint64_t n, const uint64_t* public_inputs,
                              uint64_t num_public, const uint64_t* coeffs, uint8_t* verdict);
/* the two GT values that equation compares (arkworks' 12 Fq each), for explicit coefficients and n >= 1; G16_ERR_BAD_ARG if a point
 * is off its curve, G16_ERR_UNEXPECTED_IDENTITY if the Miller product is 0 */
int g16_host_verify_aggregate_gt(int curve, const g16_vk_view* vk, const uint64_t* proofs, uint64_t n, const uint64_t* public_inputs,
                                 uint64_t num_public, const uint64_t* coeffs, uint64_t* lhs_fq12, uint64_t* rhs_fq12);
/* The aggregate equation for a batch that MIXES verifying keys: key_of[i] < n_keys names the key of proof i,
 *   FE(prod_i ML(r_i A_i, B_i) * prod_k [ML(S_IC_k, -gamma_k) * ML(S_C_k, -delta_k)]) == prod_k e(alpha_k, beta_k)^(s_k),
 *   s_k = sum_{i in k} r_i, S_IC_k = sum_{i in k} r_i IC_i, S_C_k = sum_{i in k} r_i C_i -- one final exponentiation for the call,
 * the per-key pairs and GT powers on the GPU, one lane per key.
 * proofs: n x (A | B | C) affine in the caller's order; the keys may come in any order and with any group sizes, a key with no proof
 * contributes nothing, and the same g16_pvk may be listed under several indices.
 * public_inputs: the concatenation, in proof order, of every proof's inputs -- proof i brings n_gamma_abc(key_of[i]) - 1 Fr of four
 * words; n_public_total: the caller's count of those Fr.  G16_ERR_MALFORMED_VK when it differs from the sum the keys imply (what
 * num_public + 1 != n_gamma_abc is to g16_verify_aggregate).
 * *verdict, its precedence (2 over 3 over 0 / 1), coeffs (explicit and non-zero, or NULL for getrandom(2)), the soundness contract
 * and "n = 0 gives 1" exactly as g16_verify_aggregate / g16_verify_aggregate_checked; check_subgroups != 0 runs the membership tests
 * first, on the same uploaded copy of the proofs and the same stream (verdict 3).  With n_keys = 1 the verdict is
 * g16_verify_aggregate[_checked]'s on the same coefficients.
 * G16_ERR_BAD_ARG: a key_of entry >= n_keys, n > 0 with n_keys = 0, a NULL key, a key of another curve or one loaded on another
 * context, n >= 2^32, a zero coefficient.
 * A multi-device ctx runs the whole call on its FIRST device (as g16_pairing does); a mixed batch is not cut over devices. */
int g16_verify_aggregate_mixed(g16_ctx* ctx, const g16_pvk* const* pvks, uint64_t n_keys, const uint32_t* key_of, const uint64_t* proofs,
                               uint64_t n, const uint64_t* public_inputs, uint64_t n_public_total, const uint64_t* coeffs,
                               int check_subgroups, uint8_t* verdict);
/* the same templates on the CPU (vks: n_keys views; verdicts 1 / 0 / 2) */
int g16_host_verify_aggregate_mixed(int curve, const g16_vk_view* vks, uint64_t n_keys, const uint32_t* key_of, const uint64_t* proofs,
                                    uint64_t n, const uint64_t* public_inputs, uint64_t n_public_total, const uint64_t* coeffs,
                                    uint8_t* verdict);
/* the two GT values that equation compares, for explicit coefficients and n >= 1; errors as g16_host_verify_aggregate_gt.  With
 * n_keys = 1 they are byte-equal to g16_host_verify_aggregate_gt's. */
int g16_host_verify_aggregate_mixed_gt(int curve, const g16_vk_view* vks, uint64_t n_keys, const uint32_t* key_of, const uint64_t* proofs,
                                       uint64_t n, const uint64_t* public_inputs, uint64_t n_public_total, const uint64_t* coeffs,
                                       uint64_t* lhs_fq12, uint64_t* rhs_fq12);

/* ---- the input-preparation lab (test hooks): the verifier's window tables and prepared input in place ----
 * Every verifier path first forms IC = gamma_abc_g1[0] + sum_j x_j gamma_abc_g1[j + 1] from a prepared key's window tables,
 * tables[j][w][d - 1] = d * 16^w * gamma_abc_g1[j + 1] for 64 windows w and the digits d = 1 .. 15.  These calls show both.  Points
 * leave in the ABI's G1 affine form (Montgomery limbs, the identity all-zero).
 * g16_dev_pvk_tables copies the tables of the key's copy number device_index (0 for a single-device context) back:
 * (n_gamma_abc - 1) * 64 * 15 points in the order [base][window][digit - 1]; G16_ERR_BAD_ARG for an index the key has no copy on
 * or a key of another context.  g16_dev_prepare_inputs runs one GPU lane per row of num_public Fr (inputs: n rows, Montgomery
 * limbs) on the resident tables of the key's first copy, the function the batch verifier's lanes call, and writes n points;
 * G16_ERR_MALFORMED_VK when num_public + 1 != n_gamma_abc, n = 0 is G16_OK and writes nothing, n > 2^22 is G16_ERR_BAD_ARG.
 * The g16_host_ forms build the tables on the CPU, entry by entry with the table kernel's own function, and run the same
 * accumulation (no GPU needed).  An input row is read as g16_verify_batch reads it (see there: x and x + r are the same input). */
int g16_dev_pvk_tables(g16_ctx* ctx, const g16_pvk* pvk, int device_index, uint64_t* out);
int g16_dev_prepare_inputs(g16_ctx* ctx, const g16_pvk* pvk, const uint64_t* inputs, uint64_t num_public, uint64_t n, uint64_t* out);
int g16_host_pvk_tables(int curve, const g16_vk_view* vk, uint64_t* out);
int g16_host_prepare_inputs(int curve, const g16_vk_view* vk, const uint64_t* inputs, uint64_t num_public, uint64_t n, uint64_t* out);

/* ---- prime-order subgroup membership on the GPU (the point checks of Validate::Yes, without the byte formats) ----
 * Endomorphism tests with public constants: BLS12-381 G1 phi(P) = -[x^2]P, BLS12-381 G2 psi(Q) = [x]Q,
 * BN254 G2 psi(Q) = [6x^2]Q; BN254 G1 has cofactor 1, so on-curve is membership.  A flag byte is 1: in the subgroup (the
 * identity included), 0: on the curve but outside the subgroup, 2: off the curve (as in every verifier verdict).
 * points: n packed affine points in host memory (g2 = 0: G1, 1: G2), flags: n bytes.  What Validate::Yes checks of a point
 * once its bytes are decoded; g16_deserialize_points(validate = 2) is the host path for byte input.  n = 0 is G16_OK.  A
 * multi-device ctx cuts the array into one chunk per device; flags stay in input order. */
int g16_check_subgroups(g16_ctx* ctx, int g2, const uint64_t* points, uint64_t n, uint8_t* flags);
/* proofs: n x (A | B | C) as for g16_verify_batch, uploaded once; flags[i]: 2 if any of A, B, C is off its curve, otherwise 0 if
 * any is outside its subgroup, otherwise 1 -- Validate::Yes for a whole Proof<E> (data_structures.rs:8-16). */
int g16_check_proof_subgroups(g16_ctx* ctx, const uint64_t* proofs, uint64_t n, uint8_t* flags);
/* g16_verify_aggregate with the membership tests run first, on the same uploaded copy of the proofs and the same stream: the
 * check Validate::Yes makes when the reference deserialises a proof, so the 2^-127 contract holds with NO proviso on the points.
 * *verdict as g16_verify_aggregate, plus 3: every point is on its curve but some point is outside its prime-order subgroup
 * (the equation's outcome is then not reported; g16_check_proof_subgroups names the proofs).  2 wins over 3, 3 over 0 / 1. */
int g16_verify_aggregate_checked(g16_ctx* ctx, const g16_pvk* pvk, const uint64_t* proofs, uint64_t n, const uint64_t* public_inputs,
                                 uint64_t num_public, const uint64_t* coeffs, uint8_t* verdict);
/* g16_check_subgroups' templates on the CPU (no GPU needed); the point checks of Validate::Yes */
int g16_host_check_subgroups(int curve, int g2, const uint64_t* points, uint64_t n, uint8_t* flags);

/* ---- compressed points and proofs decoded on the GPU: what Proof::deserialize_compressed reads (data_structures.rs:8-16) ----
 * The byte formats and rules are those of g16_deserialize_points(compressed = 1, validate = 0) (serialize.hip): BLS12-381 zcash
 * form (48 / 96 bytes, big-endian, flags 0x80 / 0x40 / 0x20 in the first byte, Fq2 as c1 | c0), BN254 ark-serialize form (32 / 64
 * bytes, little-endian, flags 0x80 / 0x40 in the last byte, Fq2 as c0 | c1).  One square root per point, one point per GPU lane
 * (DESIGN.md 4.6).  Where that call answers G16_ERR_INVALID_DATA for the whole array -- a coordinate >= p, BLS12-381 without the
 * compressed bit, the infinity flag with x != 0 or with the sign flag, an x with no point -- these answer per item: status 1 and the
 * affine point (byte-equal to g16_deserialize_points' output; the identity all-zero), or status 0 and the identity.  No on-curve test
 * is needed (a decoded point is on its curve by construction) and none for the subgroup is made: g16_check_subgroups does that.
 * bytes: n packed encodings in host memory (g2 = 0: G1, 1: G2), points_out: n affine points, status: n bytes.  n = 0 is G16_OK.
 * A multi-device ctx cuts the array into one chunk per device; outputs stay in input order. */
int g16_decompress_points(g16_ctx* ctx, int g2, const uint8_t* bytes, uint64_t n, uint64_t* points_out, uint8_t* status);
/* bytes: n compressed proofs A | B | C (192 / 128 bytes each; Proof<E>, data_structures.rs:8-16); proofs_out: n x (A | B | C) affine
 * as g16_verify_batch takes them; status[i]: 1 iff A, B and C all decode (a point that does not is written as the identity). */
int g16_decompress_proofs(g16_ctx* ctx, const uint8_t* bytes, uint64_t n, uint64_t* proofs_out, uint8_t* status);
/* g16_decompress_points' templates on the CPU (no GPU needed), one status byte per point */
int g16_host_decompress_points(int curve, int g2, const uint8_t* bytes, uint64_t n, uint64_t* points_out, uint8_t* status);
/* Bytes to verdict: g16_verify_aggregate_checked over compressed proofs (data_structures.rs:8-16 by the serialize.hip rules above).
 * Per device chunk the bytes are uploaded (a third of the affine form), decoded into a device buffer, and the membership tests and
 * the aggregate equation run on that buffer and the same stream; nothing returns to the host in between.
 * *verdict: 1 / 0 / 3 as g16_verify_aggregate_checked, plus 4: some proof's bytes do not decode (the equation's outcome is then not
 * reported; g16_decompress_proofs names the proofs).  4 wins over 3, 3 over 0 / 1; 2 cannot occur.  n = 0 gives 1.  Arguments,
 * coefficients, G16_ERR_MALFORMED_VK and multi-device chunking as g16_verify_aggregate. */
int g16_verify_aggregate_bytes(g16_ctx* ctx, const g16_pvk* pvk, const uint8_t* proof_bytes, uint64_t n, const uint64_t* public_inputs,
                               uint64_t num_public, const uint64_t* coeffs, uint8_t* verdict);

/* ---- a serialized proving key onto the GPU: bytes to window tables ----
 * g16_decompress_points generalised to both encodings and the three validation levels of g16_deserialize_points, one point per GPU
 * lane.  bytes: n packed encodings in host memory (g2 = 0: G1, 1: G2; compressed = 0: x | y, twice the size), points_out: n affine
 * points, status: n bytes.  Per point, where g16_deserialize_points(compressed, validate) on that one point returns G16_OK the status
 * is 1 and the point byte-equal to its output; otherwise the identity (all-zero) is stored and the status says why:
 *   0  the bytes do not decode (flags, a coordinate >= p, infinity with a non-zero coordinate, a compressed x with no point)
 *   2  decoded but off the curve          (uncompressed input with validate >= 1 only: validate = 0 makes no on-curve test)
 *   3  on the curve, outside the subgroup (validate = 2 only)
 * in that precedence.  Compressed input and the membership tests run the kernels of g16_decompress_points / g16_check_subgroups.
 * n = 0 is G16_OK.  A multi-device ctx cuts the array into one chunk per device; outputs stay in input order. */
int g16_decode_points(g16_ctx* ctx, int g2, int compressed, int validate, const uint8_t* bytes, uint64_t n, uint64_t* points_out,
                      uint8_t* status);
/* the same templates on the CPU (no GPU needed) */
int g16_host_decode_points(int curve, int g2, int compressed, int validate, const uint8_t* bytes, uint64_t n, uint64_t* points_out,
                           uint8_t* status);

/* What a ProvingKey<E> in CanonicalSerialize form holds (src/data_structures.rs:31-44, 125-143), section by section in file order:
 *   0 alpha_g1  1 beta_g2  2 gamma_g2  3 delta_g2  4 gamma_abc_g1 (Vec)  5 beta_g1  6 delta_g1
 *   7 a_query   8 b_g1_query   9 b_g2_query (Vec<G2>)   10 h_query   11 l_query          (7 .. 11: Vec)
 * A Vec is a little-endian u64 count followed by its points.  Not registered in g16_struct_size: the two functions below copy
 * min(info_size, sizeof(g16_pk_bytes_info)) bytes, like the *_sized readers. */
#define G16_PK_BYTES_SECTIONS 12
typedef struct {
    uint64_t consumed;                     /* bytes of the key (trailing bytes are not an error); 0 if the walk failed             */
    uint64_t count[G16_PK_BYTES_SECTIONS]; /* points per section, 1 for a single point; a Vec's count as its length word states it */
    int32_t bad_section;                   /* -1: nothing wrong; else the section of the first failure in file order               */
    int32_t bad_reason;                    /* the point's status 0 / 2 / 3 as g16_decode_points, or 4: the bytes end inside this
                                              section or its count does not fit what is left (bad_index and n_bad are then 0)      */
    uint64_t bad_index;                    /* index of that point within its section                                               */
    uint64_t n_bad;                        /* failing points in the whole key                                                      */
} g16_pk_bytes_info;
/* The container walk alone, on the host (no GPU needed): every count is checked against the bytes that are left, without overflow
 * and before anything is allocated.  G16_ERR_BAD_LENGTH (bad_reason 4) for a key that ends early or a count that cannot fit. */
int g16_host_pk_bytes_layout(int curve, const uint8_t* bytes, uint64_t len, int compressed, void* info, uint64_t info_size);
/* g16_pk_load from the key's bytes (what proving_key_to_bytes writes), with the five queries decoded and validated on the GPU:
 * after the walk above, the head (sections 0 .. 6, a handful of points) is read by g16_deserialize_points; each query is uploaded
 * in chunks of 2^20 points (environment G16_PK_BYTES_CHUNK, read at call time, at least 64), decoded by g16_decode_points' kernels
 * straight into one device array, membership-tested there when validate = 2, and its statuses folded into one record.  All five
 * arrays then go to g16_pk_load as device pointers (a, b_g1, b_g2 from index 1; their first points return to the host for the
 * glue) and are freed once the window tables are built: *out is an ordinary g16_pk.  The table fallbacks and the 2^27 limit are
 * g16_pk_load's.  validate as g16_deserialize_points; a key it would refuse is refused here with G16_ERR_INVALID_DATA, *out NULL,
 * nothing left allocated, and info naming the FIRST failing point in file order (whatever order the GPU met them in) and n_bad.
 * G16_ERR_BAD_LENGTH as the walk, or for an empty a_query / b_g1_query / b_g2_query.  G16_ERR_BAD_ARG (g16_last_error says why) for
 * a multi-device ctx: the bytes of a key are loaded whole, on one GPU.  info may be NULL. */
int g16_pk_load_bytes(g16_ctx* ctx, const uint8_t* bytes, uint64_t len, int compressed, int validate, g16_pk** out, void* info,
                      uint64_t info_size);
/* milliseconds the last successful g16_pk_load_bytes on this thread spent: ms[0] walk + head (host clock), ms[1] uploads, ms[2] decode
 * kernels, ms[3] membership kernels + folds (device events, summed over the chunks), ms[4] g16_pk_load (host clock; it ends in a
 * device synchronise).  Writes min(n, 5) values. */
int g16_pk_load_bytes_timings(double* ms, int n);

const char* g16_strerror(int status);
/* text of the last HIP error seen on this thread ("" if none) */
const char* g16_last_error(void);
const char* g16_version(void);
/* ABI revision of this header: bumped whenever a struct written by the library GROWS (fields are only ever appended).  2 = round 5's
 * g16_timings.g1_pass_launches and g16_pk_info.  A caller compiled against an older header must not let the library write the
 * longer struct into its shorter one: it checks g16_abi_version() == G16_ABI_VERSION at start-up, or asks for the library's struct
 * sizes (g16_struct_size), or uses the *_sized readers below, which copy min(size, library's size) bytes and never more. */
#define G16_ABI_VERSION 2
int g16_abi_version(void);
enum { G16_STRUCT_TIMINGS = 0, G16_STRUCT_PK_INFO = 1, G16_STRUCT_DIAG = 2, G16_STRUCT_PROOF = 3, G16_STRUCT_PARTIAL = 4, G16_STRUCT_PK_VIEW = 5, G16_STRUCT_VK_VIEW = 6, G16_STRUCT_CHECK_RESULT = 7,
       G16_STRUCT_PASS_LAB_JOB = 8, G16_STRUCT_SORT_LAB_INFO = 9 };
/* sizeof the library's own idea of a struct of this header; 0 for an unknown `which` */
uint64_t g16_struct_size(int which);
/* g16_get_timings / g16_pk_get_info into a caller struct of `size` bytes (its sizeof at ITS compile time) */
int g16_get_timings_sized(g16_ctx* ctx, void* out, uint64_t size);
int g16_pk_get_info_sized(const g16_pk* pk, void* out, uint64_t size);

#ifdef __cplusplus
}
#endif
#endif /* G16_MI355X_H */
