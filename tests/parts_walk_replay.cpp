// Stand-alone replay of the parts lab's job file (tests/parts_cases.py dump_jobs; tests/test_parts_host.py writes one to its temporary
// directory): every recorded job goes through g16_host_msm_parts_lab -- the layout rule and the per-task walk of
// groth16_amd/csrc/part_walk.hpp, the code the bucket pass runs per lane, compiled for the host -- and task_off, the records and the
// folded sum must equal the recorded ones bit for bit.  Meant for a sanitizer build, which cannot be had through Python: the twin
// reads the table and the sorted list through exactly sized heap copies and writes exactly sized records, so an entry index, a table
// index or a slot out of range is reported here and not by a fault on a GPU.  Compile this file together with
// groth16_amd/csrc/partslab.hip, which takes nothing from the rest of the library, e.g.
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -I include tests/parts_walk_replay.cpp groth16_amd/csrc/partslab.hip -o parts_walk_replay && ./parts_walk_replay parts_lab.bin
// It touches no GPU.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "g16_mi355x.h"

template <class T>
static bool read_n(FILE* fh, std::vector<T>& v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), fh) == v.size(); }

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s <job file>\n", argv[0]); return 2; }
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) { perror(argv[1]); return 2; }
    uint32_t hdr[14];
    unsigned long jobs = 0, tasks = 0, bad = 0;
    while (fread(hdr, sizeof(uint32_t), 14, fh) == 14) {
        const uint32_t curve = hdr[0], merged = hdr[1], c = hdr[2], groups = hdr[3], lmax = hdr[4], rows = hdr[5], base_count = hdr[6],
                       n_sorted = hdr[7], M = hdr[8], aff = hdr[9], rec = hdr[10], n_records = hdr[11];
        int64_t shift;
        memcpy(&shift, hdr + 12, sizeof(shift));
        if (M == 0 || M > (1u << 12) || n_sorted > (1u << 16) || base_count > (1u << 16) || rows > 32 || aff > 32 || rec > 128 || lmax == 0 ||
            n_records > n_sorted / lmax + M) {
            fprintf(stderr, "job %lu: bad header\n", jobs);
            return 2;
        }
        // exactly sized heap buffers: a read or a write past them is the sanitizer's to report
        std::vector<uint64_t> table((size_t)rows * base_count * aff), want_out(aff), out(aff, 0xDEADBEEFDEADBEEFull);
        std::vector<uint32_t> counts(M), sorted(n_sorted), want_task(M + 1), want_rec((size_t)n_records * rec);
        std::vector<uint32_t> offsets(M + 1), task_off(M + 1), heavy(M + 1), records((size_t)(n_sorted / lmax + M) * rec, 0xA5A5A5A5u);
        if (!read_n(fh, table) || !read_n(fh, counts) || !read_n(fh, sorted) || !read_n(fh, want_task) || !read_n(fh, want_rec) || !read_n(fh, want_out)) {
            fprintf(stderr, "job %lu: truncated\n", jobs);
            return 2;
        }
        g16_pass_lab_job job;
        memset(&job, 0, sizeof(job));
        job.table = table.data(); job.base_count = base_count; job.shift = shift; job.counts = counts.data(); job.sorted = sorted.data();
        job.n_sorted = n_sorted; job.record_cap = n_sorted / lmax + M; job.records = records.data(); job.offsets = offsets.data();
        job.task_off = task_off.data(); job.heavy = heavy.data(); job.out_affine = out.data();
        const int rc = g16_host_msm_parts_lab((int)curve, (int)merged, (int)c, (int)groups, (int)lmax, (int)rows, &job);
        if (rc != G16_OK) { fprintf(stderr, "job %lu: status %d\n", jobs, rc); ++bad; }
        else if (job.n_records != n_records || task_off != want_task || !std::equal(want_rec.begin(), want_rec.end(), records.begin()) || out != want_out) {
            fprintf(stderr, "job %lu (curve %u, merged %u, lmax %u): outputs differ from the recorded ones\n", jobs, curve, merged, lmax);
            ++bad;
        }
        ++jobs;
        tasks += n_records;
    }
    fclose(fh);
    printf("parts_walk_replay: %lu jobs, %lu tasks, %lu bad\n", jobs, tasks, bad);
    return bad || !jobs ? 1 : 0;
}
