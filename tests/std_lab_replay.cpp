// Stand-alone replay of the standard-form lab's operand file (tests/std_cases.py dump_operands; tests/test_std_cases.py writes one to
// its temporary directory): every record's tuples go through g16_host_std_op and the outputs must equal the recorded ones bit for
// bit.  Meant for a sanitizer build of the host code, which cannot be had through Python: compile this file together with
// groth16_amd/csrc/stdlab.hip, once as it is and once with -DG16_FP_PRODUCT32, which makes every product of the host compile -- the
// group law's too -- the device's 32-bit body (Fp::mul_cios32); the recorded outputs are canonical, so both must reproduce them:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         [-DG16_FP_PRODUCT32] -I include tests/std_lab_replay.cpp groth16_amd/csrc/stdlab.hip -o std_lab_replay && ./std_lab_replay std_lab.bin
// It touches no GPU: the two symbols stdlab.hip takes from the rest of the library (the context's devices, the error note) are
// stubbed here.  The signed 64-bit borrows of Fp::operator- and Fp::reduce_once are the code of interest.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "g16_mi355x.h"

namespace g16 {
int ctx_devices(const g16_ctx*, int*, std::vector<int>&, std::vector<hipStream_t>&) { return G16_ERR_BAD_ARG; }
void set_last_error(const char*, hipError_t, const char*, int) {}
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s <operand file>\n", argv[0]); return 2; }
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) { perror(argv[1]); return 2; }
    uint32_t hdr[7];
    unsigned long records = 0, tuples = 0, bad = 0;
    while (fread(hdr, sizeof(uint32_t), 7, fh) == 7) {
        const uint32_t curve = hdr[0], kind = hdr[1], form = hdr[2], n = hdr[3], nin = hdr[4], nout = hdr[5], nw = hdr[6];
        if (n == 0 || n > (1u << 22) || nin > 32 || nout > 32 || nw > 16) { fprintf(stderr, "record %lu: bad header\n", records); return 2; }
        // exactly sized heap buffers: a read or a write past a tuple's slots is the sanitizer's to report
        std::vector<uint32_t> in((size_t)n * nin * nw), want((size_t)n * nout * nw), got((size_t)n * nout * nw, 0xDEADBEEFu);
        if (fread(in.data(), sizeof(uint32_t), in.size(), fh) != in.size() || fread(want.data(), sizeof(uint32_t), want.size(), fh) != want.size()) {
            fprintf(stderr, "record %lu: truncated\n", records);
            return 2;
        }
        const int rc = g16_host_std_op((int)curve, (int)kind, (int)form, in.data(), n, got.data());
        if (rc != G16_OK) { fprintf(stderr, "curve %u kind %u form %u: status %d\n", curve, kind, form, rc); ++bad; }
        else if (memcmp(got.data(), want.data(), want.size() * sizeof(uint32_t)) != 0) { fprintf(stderr, "curve %u kind %u form %u: outputs differ from the recorded ones\n", curve, kind, form); ++bad; }
        ++records;
        tuples += n;
    }
    fclose(fh);
#ifdef G16_FP_PRODUCT32
    const char* body = "32-bit product everywhere";
#else
    const char* body = "64-bit host product";
#endif
    printf("std_lab_replay (%s): %lu records, %lu tuples, %lu bad\n", body, records, tuples, bad);
    return bad || !records ? 1 : 0;
}
