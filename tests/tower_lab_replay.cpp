// Stand-alone replay of the tower lab's operand file (tests/tower_cases.py dump_operands; tests/test_tower_host.py writes one to its
// temporary directory): every record's tuples go through g16_host_pairing_op and the outputs must equal the recorded ones bit for
// bit.  Meant for a sanitizer build of the host code, which cannot be had through Python: compile this file together with
// groth16_amd/csrc/towerlab.hip, e.g.
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -I include tests/tower_lab_replay.cpp groth16_amd/csrc/towerlab.hip -o tower_lab_replay && ./tower_lab_replay tower_lab.bin
// It touches no GPU: the two symbols towerlab.hip takes from the rest of the library (the context's devices, the error note) are
// stubbed here.
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
    uint32_t hdr[6];
    unsigned long records = 0, tuples = 0, bad = 0;
    while (fread(hdr, sizeof(uint32_t), 6, fh) == 6) {
        const uint32_t curve = hdr[0], form = hdr[1], n = hdr[2], nin = hdr[3], nout = hdr[4], nl = hdr[5];
        if (n == 0 || n > (1u << 22) || nin > 64 || nout > 64 || nl > 16) { fprintf(stderr, "record %lu: bad header\n", records); return 2; }
        // exactly sized heap buffers: a read or a write past a tuple's slots is the sanitizer's to report
        std::vector<uint32_t> in((size_t)n * nin * nl), want((size_t)n * nout * nl), got((size_t)n * nout * nl, 0xDEADBEEFu);
        if (fread(in.data(), sizeof(uint32_t), in.size(), fh) != in.size() || fread(want.data(), sizeof(uint32_t), want.size(), fh) != want.size()) {
            fprintf(stderr, "record %lu: truncated\n", records);
            return 2;
        }
        const int rc = g16_host_pairing_op((int)curve, (int)form, in.data(), n, got.data());
        if (rc != G16_OK) { fprintf(stderr, "curve %u form %u: status %d\n", curve, form, rc); ++bad; }
        else if (memcmp(got.data(), want.data(), want.size() * sizeof(uint32_t)) != 0) { fprintf(stderr, "curve %u form %u: outputs differ from the recorded ones\n", curve, form); ++bad; }
        ++records;
        tuples += n;
    }
    fclose(fh);
    printf("tower_lab_replay: %lu records, %lu tuples, %lu bad\n", records, tuples, bad);
    return bad || !records ? 1 : 0;
}
