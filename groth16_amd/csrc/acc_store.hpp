// Where the bucket pass and the bucket reduction park an accumulator's coordinates in LDS; shared with the field lab (devtest.hip),
// which runs AccParked over the same layout.
#pragma once
#include "hd.hpp"
#include <cstdint>

namespace g16 {

static constexpr int ACC_THREADS = 64;   // one wave per workgroup: finer re-dispatch granularity.  Same box, full proof at 2^22 (round 3): 64 lanes
                                         // 79.56 ms (G2 pass 25.87), 128 lanes 80.38 / 80.17 (26.53 / 26.44), 256 lanes 80.81 (26.76); G1 passes equal

// The accumulator's coordinates in LDS (AccParked, fp30.hpp): value v, limb i of lane t.  Limbs are grouped in fours so that a
// coordinate moves as ds_read_b128 / ds_write_b128 (each lane its own 16 bytes, consecutive lanes consecutive: conflict-free) plus
// single words for the NL mod 4 tail rows.  4 * NL * 64 words per 64-lane workgroup: 13 KB (NL = 13), i.e. 104 of the CU's 160 KB at
// two waves per SIMD (eight workgroups per CU).
template <class F30>
struct LdsAccStore {
    static constexpr int NL = F30::PREFIX_LIMBS;
    static constexpr int QUADS = NL / 4, TAIL = NL % 4;
    static constexpr int WORDS_PER_VALUE = NL * ACC_THREADS;
    uint32_t* quad;   // lds + 4 * lane
    uint32_t* tail;   // lds + 4 * QUADS * ACC_THREADS + lane
    __device__ __forceinline__ F30 ld(int v) const {
        asm volatile("" ::: "memory");   // a FRESH read every time: the point of parking is that the value is not kept live
        uint32_t w[NL];
        const uint32_t* q = quad + v * WORDS_PER_VALUE;
        G16_UNROLL for (int g = 0; g < QUADS; ++g) {
            const uint4 t = *reinterpret_cast<const uint4*>(q + g * 4 * ACC_THREADS);
            w[4 * g] = t.x; w[4 * g + 1] = t.y; w[4 * g + 2] = t.z; w[4 * g + 3] = t.w;
        }
        const uint32_t* r = tail + v * WORDS_PER_VALUE;
        G16_UNROLL for (int i = 0; i < TAIL; ++i) w[4 * QUADS + i] = r[i * ACC_THREADS];
        return F30::from_limbs(w);
    }
    __device__ __forceinline__ void st(int v, const F30& a) const {
        uint32_t w[NL];
        a.get_limbs(w);
        uint32_t* q = quad + v * WORDS_PER_VALUE;
        G16_UNROLL for (int g = 0; g < QUADS; ++g)
            *reinterpret_cast<uint4*>(q + g * 4 * ACC_THREADS) = make_uint4(w[4 * g], w[4 * g + 1], w[4 * g + 2], w[4 * g + 3]);
        uint32_t* r = tail + v * WORDS_PER_VALUE;
        G16_UNROLL for (int i = 0; i < TAIL; ++i) r[i * ACC_THREADS] = w[4 * QUADS + i];
        asm volatile("" ::: "memory");
    }
};

}  // namespace g16
