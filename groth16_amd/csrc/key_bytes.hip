// A serialized proving key onto the GPU: bytes to the device arrays g16_pk_load builds its window tables from.
//
//   keyload_decode_g1_kernel / keyload_decode_g2_kernel   the UNCOMPRESSED forms (Decompress<C>::g1_raw / g2_raw): lane i reads the
//                              encoding at in + i * in_stride (bytes), range-checks the coordinates, makes the on-curve test when asked
//                              to and stores the affine point at out + i * out_stride (64-bit words) and one status byte (1 / 0 / 2;
//                              the identity is stored unless the status is 1).  No square root, no LDS, nothing shared between lanes.
//   keyload_fold_kernel        one lane per point: the decode status and (validate = 2) the membership flag become the point's final
//                              status 1 / 0 / 2 / 3, a point outside its subgroup is overwritten with the identity, and the chunk's
//                              failures are folded into the query's record in HBM -- the count and the minimum of (index << 2 | status).
//                              As r1cs_check_kernel: one ballot per wave, one lane of a wave that saw a failure speaks for it; count and
//                              minimum do not depend on the order the waves arrive in.
// The COMPRESSED forms and the membership tests are the kernels of verify_decompress.hip / verify_subgroup.hip, launched through
// decompress_enqueue_points / subgroup_enqueue_points: no second instantiation of the square-root and endomorphism chains.
// g16_host_decode_points runs the same templates on the CPU.
#include "decompress.hpp"
#include "subgroup.hpp"
#include "verify_common.hpp"
#include <chrono>

using namespace g16;

namespace g16 {

// Waves per SIMD the decode is compiled for: a lane holds one point and the temporaries of the curve equation's products
constexpr int KEYLOAD_WAVES = 4;
constexpr int FOLD_BLOCK = 256;
constexpr uint64_t KEY_CHUNK_DEFAULT = (uint64_t)1 << 20, KEY_CHUNK_MIN = 64;

template <class C>
__global__ __launch_bounds__(VERIFY_BLOCK, KEYLOAD_WAVES) void keyload_decode_g1_kernel(const uint8_t* in, uint64_t in_stride, uint64_t* out,
                                                                                        uint64_t out_stride, uint64_t n, int check_curve,
                                                                                        uint8_t* status) {
    const uint64_t i = (uint64_t)blockIdx.x * VERIFY_BLOCK + threadIdx.x;
    if (i >= n) return;
    typename C::G1A p;
    status[i] = Decompress<C>::g1_raw(in + i * in_stride, check_curve != 0, &p);
    __builtin_memcpy(out + i * out_stride, &p, sizeof(p));
}

template <class C>
__global__ __launch_bounds__(VERIFY_BLOCK, KEYLOAD_WAVES) void keyload_decode_g2_kernel(const uint8_t* in, uint64_t in_stride, uint64_t* out,
                                                                                        uint64_t out_stride, uint64_t n, int check_curve,
                                                                                        uint8_t* status) {
    const uint64_t i = (uint64_t)blockIdx.x * VERIFY_BLOCK + threadIdx.x;
    if (i >= n) return;
    // decoded in place (g2_raw): out and out_stride are 16-byte aligned, as every point array the host side of this file allocates
    status[i] = Decompress<C>::g2_raw(in + i * in_stride, check_curve != 0, reinterpret_cast<typename C::G2A*>(out + i * out_stride));
}

// status: n decode statuses in, final statuses out; flags: n membership flags, or null (validate < 2); points: n x words, packed;
// base: index of point 0 within its query; rec (may be null): rec[0] += failing points, rec[1] = min(rec[1], index << 2 | status)
// (the host zeroes rec[0] and sets rec[1] to UINT64_MAX)
__global__ __launch_bounds__(FOLD_BLOCK) void keyload_fold_kernel(uint8_t* status, const uint8_t* flags, uint64_t* points, uint32_t words,
                                                                  uint64_t n, uint64_t base, unsigned long long* rec) {
    const uint64_t i = (uint64_t)blockIdx.x * FOLD_BLOCK + threadIdx.x;
    uint8_t st = 1;
    if (i < n) {
        st = status[i];
        if (flags) {
            const uint8_t merged = decode_status_with_flag(st, flags[i]);
            if (merged != st) {
                st = merged;
                status[i] = st;
                uint64_t* p = points + i * words;
                for (uint32_t k = 0; k < words; ++k) p[k] = 0;
            }
        }
    }
    const unsigned long long m = __ballot(st != 1);   // wave64: one bit per lane, indices ascend with the lane
    if (m == 0 || !rec) return;
    if ((threadIdx.x & 63u) == (unsigned)(__ffsll((long long)m) - 1)) {   // the wave's first failure speaks for the wave
        atomicAdd(&rec[0], (unsigned long long)__popcll(m));
        atomicMin(&rec[1], (unsigned long long)(((base + i) << 2) | st));
    }
}

template <class C>
int enqueue_raw(hipStream_t s, int g2, int check_curve, const uint8_t* d_bytes, uint64_t n, uint64_t* d_points, uint8_t* d_status) {
    constexpr int L = C::Fq::N / 2;
    constexpr uint64_t FB = Decompress<C>::FQ_BYTES;
    const uint64_t blocks = (n + VERIFY_BLOCK - 1) / VERIFY_BLOCK;
    if (blocks > 0x7fffffffull) return G16_ERR_BAD_ARG;
    if (g2) keyload_decode_g2_kernel<C><<<(unsigned)blocks, VERIFY_BLOCK, 0, s>>>(d_bytes, 4 * FB, d_points, 4 * L, n, check_curve, d_status);
    else keyload_decode_g1_kernel<C><<<(unsigned)blocks, VERIFY_BLOCK, 0, s>>>(d_bytes, 2 * FB, d_points, 2 * L, n, check_curve, d_status);
    G16_LAUNCH_CHECK();
    return G16_OK;
}

inline uint64_t point_words(int curve, int g2) { return (uint64_t)(curve == G16_BLS12_381 ? 12 : 8) * (g2 ? 2 : 1); }

// events around the three stages of a chunk, read once the stream has been waited for (null: no timing)
struct StageClock {
    std::vector<hipEvent_t> ev;   // four per chunk: before the upload, after it, after the decode, after membership + fold
    ~StageClock() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
    int mark(hipStream_t s) {
        hipEvent_t e = nullptr;
        G16_HIP_TRY(hipEventCreate(&e));
        ev.push_back(e);
        G16_HIP_TRY(hipEventRecord(e, s));
        return G16_OK;
    }
    void sums(double out[3]) const {
        out[0] = out[1] = out[2] = 0.0;
        for (size_t k = 0; k + 3 < ev.size(); k += 4)
            for (int j = 0; j < 3; ++j) {
                float t = 0.f;
                if (hipEventElapsedTime(&t, ev[k + j], ev[k + j + 1]) == hipSuccess) out[j] += t;
            }
    }
};

// Everything one chunk needs, queued on s: n encodings at `bytes` (host) -> d_bytes -> d_points (n x words, written in place) with
// the final statuses in d_status.  d_flags: n bytes of work space (validate = 2).  base, d_rec: as keyload_fold_kernel.
int enqueue_chunk(hipStream_t s, int curve, int g2, int compressed, int validate, const uint8_t* bytes, uint8_t* d_bytes, uint64_t n,
                  uint64_t base, uint64_t* d_points, uint8_t* d_status, uint8_t* d_flags, unsigned long long* d_rec, StageClock* clock) {
    const uint64_t esz = serialized_point_size(curve, g2, compressed);
    if (clock) G16_TRY(clock->mark(s));
    G16_HIP_TRY(hipMemcpyAsync(d_bytes, bytes, n * esz, hipMemcpyHostToDevice, s));
    if (clock) G16_TRY(clock->mark(s));
    if (compressed) {
        G16_TRY(decompress_enqueue_points(s, curve, g2, d_bytes, n, d_points, d_status));
    } else if (curve == G16_BLS12_381) {
        G16_TRY(enqueue_raw<Bls12_381>(s, g2, validate >= 1, d_bytes, n, d_points, d_status));
    } else {
        G16_TRY(enqueue_raw<Bn254>(s, g2, validate >= 1, d_bytes, n, d_points, d_status));
    }
    if (clock) G16_TRY(clock->mark(s));
    if (validate >= 2) G16_TRY(subgroup_enqueue_points(s, curve, g2, d_points, n, d_flags));
    if (validate >= 2 || d_rec) {
        const uint64_t blocks = (n + FOLD_BLOCK - 1) / FOLD_BLOCK;
        if (blocks > 0x7fffffffull) return G16_ERR_BAD_ARG;
        keyload_fold_kernel<<<(unsigned)blocks, FOLD_BLOCK, 0, s>>>(d_status, validate >= 2 ? d_flags : nullptr, d_points,
                                                                    (uint32_t)point_words(curve, g2), n, base, d_rec);
        G16_LAUNCH_CHECK();
    }
    if (clock) G16_TRY(clock->mark(s));
    return G16_OK;
}

int decode_points_device(g16_ctx* ctx, int g2, int compressed, int validate, const uint8_t* bytes, uint64_t n, uint64_t* out, uint8_t* status) {
    CtxView cv;
    G16_TRY(cv.load(ctx));
    if (cv.curve != G16_BLS12_381 && cv.curve != G16_BN254) return G16_ERR_BAD_ARG;
    const uint64_t esz = serialized_point_size(cv.curve, g2, compressed), words = point_words(cv.curve, g2);
    return for_each_chunk(cv, n, [&](uint64_t k, uint64_t lo, uint64_t cnt, DevBufs& bufs) -> int {
        hipStream_t s = cv.streams[k];
        G16_HIP_TRY(hipSetDevice(cv.devs[k]));
        uint8_t *d_in, *d_status, *d_flags;
        uint64_t* d_out;
        G16_TRY(bufs.get(&d_in, cnt * esz));
        G16_TRY(bufs.get(&d_out, cnt * words));
        G16_TRY(bufs.get(&d_status, cnt));
        G16_TRY(bufs.get(&d_flags, cnt));
        G16_TRY(enqueue_chunk(s, cv.curve, g2, compressed, validate, bytes + lo * esz, d_in, cnt, lo, d_out, d_status, d_flags, nullptr, nullptr));
        G16_HIP_TRY(hipMemcpyAsync(out + lo * words, d_out, cnt * words * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        G16_HIP_TRY(hipMemcpyAsync(status + lo, d_status, cnt, hipMemcpyDeviceToHost, s));
        return G16_OK;
    });
}

template <class C>
int host_decode_any(int g2, int compressed, int validate, const uint8_t* bytes, uint64_t n, uint64_t* out, uint8_t* status) {
    constexpr int L = C::Fq::N / 2;
    typedef Decompress<C> D;
    const uint64_t esz = serialized_point_size(C::CURVE_ID, g2, compressed);
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t* in = bytes + i * esz;
        if (g2) {
            typename C::G2A p;
            uint8_t st = compressed ? D::g2(in, &p) : D::g2_raw(in, validate >= 1, &p);
            if (validate >= 2) st = decode_status_with_flag(st, Subgroup<C>::g2_flag(p));
            if (st != 1) p = C::G2A::identity();
            status[i] = st;
            memcpy(out + i * 4 * L, &p, sizeof(p));
        } else {
            typename C::G1A p;
            uint8_t st = compressed ? D::g1(in, &p) : D::g1_raw(in, validate >= 1, &p);
            if (validate >= 2) st = decode_status_with_flag(st, Subgroup<C>::g1_flag(p));
            if (st != 1) p = C::G1A::identity();
            status[i] = st;
            memcpy(out + i * 2 * L, &p, sizeof(p));
        }
    }
    return G16_OK;
}

int host_decode_points(int curve, int g2, int compressed, int validate, const uint8_t* bytes, uint64_t n, uint64_t* out, uint8_t* status) {
    G16_VERIFY_DISPATCH(curve, (host_decode_any<CC>(g2, compressed, validate, bytes, n, out, status)));
}

// ---- the container ----------------------------------------------------------------------------------------------------------------
constexpr int N_SEC = G16_PK_BYTES_SECTIONS, FIRST_QUERY = 7;
constexpr bool SEC_G2[N_SEC] = {false, true, true, true, false, false, false, false, false, true, false, false};
constexpr bool SEC_VEC[N_SEC] = {false, false, false, false, true, false, false, true, true, true, true, true};

struct Section { uint64_t off = 0, count = 0; };

void info_clear(g16_pk_bytes_info* info) {
    memset(info, 0, sizeof(*info));
    info->bad_section = -1;
}

void info_copy_out(const g16_pk_bytes_info& info, void* out, uint64_t size) {
    if (out) memcpy(out, &info, (size_t)std::min<uint64_t>(size, sizeof(info)));
}

// offsets and counts of the twelve sections; every count is held against the bytes that are left before it is believed
int walk_key(int curve, const uint8_t* bytes, uint64_t len, int compressed, Section sec[N_SEC], g16_pk_bytes_info* info) {
    info_clear(info);
    uint64_t pos = 0;
    for (int k = 0; k < N_SEC; ++k) {
        auto fail = [&]() {
            info->bad_section = k;
            info->bad_reason = 4;
            return G16_ERR_BAD_LENGTH;
        };
        uint64_t n = 1;
        if (SEC_VEC[k]) {
            if (len - pos < 8) return fail();
            n = 0;
            for (int b = 7; b >= 0; --b) n = (n << 8) | bytes[pos + b];
            pos += 8;
        }
        info->count[k] = n;
        const uint64_t esz = serialized_point_size(curve, SEC_G2[k], compressed);
        if (n > (len - pos) / esz) return fail();   // (no product that could overflow)
        sec[k].off = pos;
        sec[k].count = n;
        pos += n * esz;
    }
    info->consumed = pos;
    return G16_OK;
}

static thread_local double g_load_ms[5] = {0, 0, 0, 0, 0};

// what the caller of g16_pk_load_bytes gets when a point fails: the first failure in file order and the number of failures
struct Failures {
    g16_pk_bytes_info* info;
    void add(int section, uint64_t index, int reason, uint64_t count) {
        if (!count) return;
        if (info->bad_section < 0) {   // sections are visited in file order
            info->bad_section = section;
            info->bad_index = index;
            info->bad_reason = reason;
        }
        info->n_bad += count;
    }
};

int load_key_bytes(g16_ctx* ctx, int curve, int device, hipStream_t s, const uint8_t* bytes, uint64_t len, int compressed, int validate,
                   g16_pk** out, g16_pk_bytes_info* info) {
    typedef std::chrono::steady_clock Clock;
    const Clock::time_point t0 = Clock::now();
    Section sec[N_SEC];
    G16_TRY(walk_key(curve, bytes, len, compressed, sec, info));
    for (int k : {7, 8, 9})   // their first points are the glue's (calculate_coeff, prover.rs:261)
        if (sec[k].count == 0) {
            info->bad_section = k;
            info->bad_reason = 4;
            info->consumed = 0;
            return G16_ERR_BAD_LENGTH;
        }
    Failures bad{info};

    // the head: a handful of points, by the host reader; if it refuses one, the templates the GPU runs say which and why
    std::vector<uint64_t> head[FIRST_QUERY];
    for (int k = 0; k < FIRST_QUERY; ++k) {
        const uint64_t words = point_words(curve, SEC_G2[k]);
        head[k].assign(std::max<uint64_t>(sec[k].count, 1) * words, 0);
        const int rc = deserialize_points(curve, SEC_G2[k], compressed, bytes + sec[k].off, sec[k].count, validate, head[k].data());
        if (rc == G16_OK) continue;
        if (rc != G16_ERR_INVALID_DATA) return rc;
        std::vector<uint8_t> st(sec[k].count, 1);
        G16_TRY(host_decode_points(curve, SEC_G2[k], compressed, validate, bytes + sec[k].off, sec[k].count, head[k].data(), st.data()));
        uint64_t first = 0, n_bad = 0;
        for (uint64_t i = sec[k].count; i-- > 0;)
            if (st[i] != 1) { first = i; ++n_bad; }
        if (n_bad) bad.add(k, first, st[first], n_bad);
        else bad.add(k, 0, 0, 1);   // (the reader and the templates disagree: tests/test_key_bytes_host.py holds them together)
    }
    const Clock::time_point t1 = Clock::now();

    // the five queries: bytes up, points decoded and checked in place, one record each
    uint64_t chunk = KEY_CHUNK_DEFAULT;
    if (const char* e = getenv("G16_PK_BYTES_CHUNK")) chunk = std::max<uint64_t>(strtoull(e, nullptr, 10), KEY_CHUNK_MIN);
    G16_HIP_TRY(hipSetDevice(device));
    DevBufs bufs;   // freed on every way out
    StageClock clock;
    uint64_t* d_q[N_SEC] = {};
    unsigned long long* d_rec = nullptr;
    unsigned long long rec[2 * N_SEC];
    for (int k = 0; k < N_SEC; ++k) { rec[2 * k] = 0; rec[2 * k + 1] = ~0ull; }
    uint64_t max_chunk = 0, max_bytes = 0;
    for (int k = FIRST_QUERY; k < N_SEC; ++k) {
        const uint64_t c = std::min(chunk, sec[k].count);
        max_chunk = std::max(max_chunk, c);
        max_bytes = std::max(max_bytes, c * serialized_point_size(curve, SEC_G2[k], compressed));
    }
    uint8_t *d_bytes, *d_status, *d_flags;
    auto enqueue_all = [&]() -> int {
        G16_TRY(bufs.get(&d_rec, 2 * N_SEC));
        G16_TRY(bufs.get(&d_bytes, max_bytes));
        G16_TRY(bufs.get(&d_status, max_chunk));
        G16_TRY(bufs.get(&d_flags, max_chunk));
        G16_HIP_TRY(hipMemcpyAsync(d_rec, rec, sizeof(rec), hipMemcpyHostToDevice, s));
        for (int k = FIRST_QUERY; k < N_SEC; ++k) {
            const uint64_t words = point_words(curve, SEC_G2[k]), esz = serialized_point_size(curve, SEC_G2[k], compressed);
            G16_TRY(bufs.get(&d_q[k], sec[k].count * words));
            for (uint64_t lo = 0; lo < sec[k].count; lo += chunk) {
                const uint64_t cnt = std::min(chunk, sec[k].count - lo);
                G16_TRY(enqueue_chunk(s, curve, SEC_G2[k], compressed, validate, bytes + sec[k].off + lo * esz, d_bytes, cnt, lo,
                                      d_q[k] + lo * words, d_status, d_flags, d_rec + 2 * k, &clock));
            }
        }
        G16_HIP_TRY(hipMemcpyAsync(rec, d_rec, sizeof(rec), hipMemcpyDeviceToHost, s));
        return G16_OK;
    };
    const int rc_q = enqueue_all();
    const bool waited = hipStreamSynchronize(s) == hipSuccess;   // before anything queued above loses its memory
    if (rc_q != G16_OK) return rc_q;
    if (!waited) return G16_ERR_HIP;
    for (int k = FIRST_QUERY; k < N_SEC; ++k)
        if (rec[2 * k]) {
            if (rec[2 * k + 1] == ~0ull || (rec[2 * k + 1] >> 2) >= sec[k].count) return G16_ERR_INTERNAL;   // a count without a point
            bad.add(k, rec[2 * k + 1] >> 2, (int)(rec[2 * k + 1] & 3), rec[2 * k]);
        }
    if (info->bad_section >= 0) return G16_ERR_INVALID_DATA;

    // the glue's three points back to the host, and the arrays to the table builder as they lie
    const uint64_t w1 = point_words(curve, 0), w2 = point_words(curve, 1);
    std::vector<uint64_t> a0(w1), b10(w1), b20(w2);
    G16_HIP_TRY(hipMemcpy(a0.data(), d_q[7], w1 * 8, hipMemcpyDeviceToHost));
    G16_HIP_TRY(hipMemcpy(b10.data(), d_q[8], w1 * 8, hipMemcpyDeviceToHost));
    G16_HIP_TRY(hipMemcpy(b20.data(), d_q[9], w2 * 8, hipMemcpyDeviceToHost));
    g16_pk_view v;
    memset(&v, 0, sizeof(v));
    v.alpha_g1 = head[0].data();
    v.beta_g2 = head[1].data();
    v.delta_g2 = head[3].data();
    v.beta_g1 = head[5].data();
    v.delta_g1 = head[6].data();
    v.a_query0 = a0.data();
    v.b_g1_query0 = b10.data();
    v.b_g2_query0 = b20.data();
    v.a = {d_q[7] + w1, sec[7].count - 1, 0};
    v.b_g1 = {d_q[8] + w1, sec[8].count - 1, 0};
    v.b_g2 = {d_q[9] + w2, sec[9].count - 1, 0};
    v.h = {d_q[10], sec[10].count, 0};
    v.l = {d_q[11], sec[11].count, 0};
    v.flags = G16_PK_DEVICE_PTRS;
    const Clock::time_point t2 = Clock::now();
    G16_TRY(g16_pk_load(ctx, &v, out));   // waits for its builds: the arrays can go when it returns
    const Clock::time_point t3 = Clock::now();
    double stage[3];
    clock.sums(stage);
    g_load_ms[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
    g_load_ms[1] = stage[0];
    g_load_ms[2] = stage[1];
    g_load_ms[3] = stage[2];
    g_load_ms[4] = std::chrono::duration<double, std::milli>(t3 - t2).count();
    return G16_OK;
}

// api.hip's g16_pk_load_bytes, once it has looked at the context
int pk_load_bytes(g16_ctx* ctx, int curve, int device, hipStream_t s, const uint8_t* bytes, uint64_t len, int compressed, int validate,
                  g16_pk** out, void* info_out, uint64_t info_size) {
    g16_pk_bytes_info info;
    info_clear(&info);
    int rc;
    try {
        rc = load_key_bytes(ctx, curve, device, s, bytes, len, compressed, validate, out, &info);
    } catch (const std::bad_alloc&) {
        rc = G16_ERR_OOM;
    } catch (...) {
        rc = G16_ERR_INTERNAL;
    }
    if (rc != G16_OK) info.consumed = 0;
    info_copy_out(info, info_out, info_size);
    return rc;
}

}  // namespace g16

extern "C" {

int g16_decode_points(g16_ctx* ctx, int g2, int compressed, int validate, const uint8_t* bytes, uint64_t n, uint64_t* points_out,
                      uint8_t* status) {
    if (!ctx || (g2 != 0 && g2 != 1) || (compressed != 0 && compressed != 1) || validate < 0 || validate > 2) return G16_ERR_BAD_ARG;
    if (n && (!bytes || !points_out || !status)) return G16_ERR_BAD_ARG;
    if (!n) return G16_OK;
    try {
        return decode_points_device(ctx, g2, compressed, validate, bytes, n, points_out, status);
    } catch (const std::bad_alloc&) {
        return G16_ERR_OOM;
    } catch (...) {
        return G16_ERR_INTERNAL;
    }
}

int g16_host_decode_points(int curve, int g2, int compressed, int validate, const uint8_t* bytes, uint64_t n, uint64_t* points_out,
                           uint8_t* status) {
    if ((g2 != 0 && g2 != 1) || (compressed != 0 && compressed != 1) || validate < 0 || validate > 2) return G16_ERR_BAD_ARG;
    if (curve != G16_BLS12_381 && curve != G16_BN254) return G16_ERR_BAD_ARG;
    if (n && (!bytes || !points_out || !status)) return G16_ERR_BAD_ARG;
    if (!n) return G16_OK;
    return host_decode_points(curve, g2, compressed, validate, bytes, n, points_out, status);
}

int g16_host_pk_bytes_layout(int curve, const uint8_t* bytes, uint64_t len, int compressed, void* info, uint64_t info_size) {
    if ((curve != G16_BLS12_381 && curve != G16_BN254) || (!bytes && len) || (compressed != 0 && compressed != 1)) return G16_ERR_BAD_ARG;
    g16_pk_bytes_info full;
    Section sec[N_SEC];
    const int rc = walk_key(curve, bytes, len, compressed, sec, &full);
    info_copy_out(full, info, info_size);
    return rc;
}

int g16_pk_load_bytes_timings(double* ms, int n) {
    if (!ms || n < 0) return G16_ERR_BAD_ARG;
    for (int k = 0; k < n && k < 5; ++k) ms[k] = g_load_ms[k];
    return G16_OK;
}

}  // extern "C"
