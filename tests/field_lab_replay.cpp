// Stand-alone replay of the field lab's operand file for the inversion, doubling and affine-pair forms (tests/table_cases.py
// dump_operands; tests/test_table_cases.py writes one to its temporary directory): every record's tuples go through g16_host_fp30_op
// and the outputs must equal the recorded ones bit for bit.  Meant for a sanitizer build of the host code, which cannot be had through
// Python -- ModInv30 is signed 32- and 64-bit limb arithmetic throughout, and a signed overflow there is undefined behaviour that a
// value check can miss on one compiler and not on the next: compile this file together with groth16_amd/csrc/devtest.hip, e.g.
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -I include tests/field_lab_replay.cpp groth16_amd/csrc/devtest.hip -o field_lab_replay && ./field_lab_replay field_lab.bin
// It touches no GPU: the two symbols devtest.hip takes from the rest of the library (the context's devices, the error note) are
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
    uint32_t hdr[7];
    unsigned long records = 0, tuples = 0, bad = 0;
    while (fread(hdr, sizeof(uint32_t), 7, fh) == 7) {
        const uint32_t curve = hdr[0], field = hdr[1], form = hdr[2], n = hdr[3], nin = hdr[4], nout = hdr[5], nl = hdr[6];
        if (n == 0 || n > (1u << 22) || nin > 64 || nout > 64 || nl > 16) { fprintf(stderr, "record %lu: bad header\n", records); return 2; }
        // exactly sized heap buffers: a read or a write past a tuple's slots is the sanitizer's to report
        std::vector<uint32_t> in((size_t)n * nin * nl), want((size_t)n * nout * nl), got((size_t)n * nout * nl, 0xDEADBEEFu);
        if (fread(in.data(), sizeof(uint32_t), in.size(), fh) != in.size() || fread(want.data(), sizeof(uint32_t), want.size(), fh) != want.size()) {
            fprintf(stderr, "record %lu: truncated\n", records);
            return 2;
        }
        const int rc = g16_host_fp30_op((int)curve, (int)field, (int)form, in.data(), n, got.data());
        if (rc != G16_OK) { fprintf(stderr, "curve %u field %u form %u: status %d\n", curve, field, form, rc); ++bad; }
        else if (memcmp(got.data(), want.data(), want.size() * sizeof(uint32_t)) != 0) {
            fprintf(stderr, "curve %u field %u form %u: outputs differ from the recorded ones\n", curve, field, form);
            ++bad;
        }
        ++records;
        tuples += n;
    }
    fclose(fh);
    printf("field_lab_replay: %lu records, %lu tuples, %lu bad\n", records, tuples, bad);
    return bad || !records ? 1 : 0;
}
