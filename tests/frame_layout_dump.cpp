// frame_layout_dump.cpp — prints what rayn_amd/csrc/frame_layout.h decides, for tests/test_frame_layout.py.  Host code only: built with
// hipcc -x hip --cuda-host-only, it calls nothing of the HIP runtime and runs without a GPU.
//   carve CAP max_tiles total_tiles NS max_bounces   "<piece> <offset>" per piece of carve(), then "total <bytes>" and "dry_total <bytes>"
//   per_path NS                                      arena_bytes_per_path
//   ids NS slots                                     queue_ids_fit, 0 or 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../rayn_amd/csrc/frame_layout.h"

using namespace rayn;

int main(int argc, char** argv) {
    const auto arg = [&](int i) { return (size_t)strtoull(argv[i], nullptr, 10); };
    if (argc == 7 && !strcmp(argv[1], "carve")) {
        // Offsets: carved over a made-up base address - nothing is dereferenced.  The total once more from an Arena without memory, the dry run that sizes
        // run_worker's allocation.
        Arena A, dry;
        A.base = (char*)(uintptr_t)0x10000000; A.cap = ~(size_t)0;
        Layout L, D;
        const size_t total = carve(A, arg(2), arg(3), arg(4), (uint32_t)arg(5), (uint32_t)arg(6), &L);
        const size_t dry_total = carve(dry, arg(2), arg(3), arg(4), (uint32_t)arg(5), (uint32_t)arg(6), &D);
#define PIECE(member) printf(#member " %zu\n", (size_t)((const char*)L.member - A.base))
        PIECE(pool.geo0); PIECE(pool.geo1); PIECE(pool.col0); PIECE(pool.col1); PIECE(pool.aov); PIECE(pool.term_key); PIECE(pool.term_info);
        PIECE(q); PIECE(qn); PIECE(bq);
        PIECE(qt.ent_obj); PIECE(qt.alive); PIECE(qt.grp_cnt); PIECE(qt.grp_base); PIECE(qt.grp_tile); PIECE(qt.bgrp_cnt); PIECE(qt.bgrp_base); PIECE(qt.bgrp_tile);
        PIECE(qt.ray_tgb); PIECE(qt.ray_tgc); PIECE(qt.bin_tgb); PIECE(qt.bin_tgc);
        PIECE(qt.tile_total); PIECE(qt.tile_valid); PIECE(qt.tile_out_base); PIECE(qt.tile_cls_cnt); PIECE(qt.tile_cls_base);
        PIECE(d_all_tiles); PIECE(pgrp_tile); PIECE(base_hist);
        PIECE(nee.x); PIECE(nee.vtr); PIECE(nee.pdf); PIECE(nee.aux); PIECE(nee.vis); PIECE(nee.vpicks); PIECE(nee.T); PIECE(nee.t0); PIECE(nee.nthr); PIECE(nee.flags);
        PIECE(nee.job_ref); PIECE(nee.job_geo);
#undef PIECE
        printf("total %zu\ndry_total %zu\n", total, dry_total);
        printf("caps %zu %zu %zu %zu %zu\n", L.QCAP, L.BCAP, L.nee.cap, L.nee.jobcap, L.hist_stride);
        return D.pool.geo0 || D.nee.job_geo ? 1 : 0; // an Arena without memory hands out no address
    }
    if (argc == 3 && !strcmp(argv[1], "per_path")) { printf("%zu\n", arena_bytes_per_path((uint32_t)arg(2))); return 0; }
    if (argc == 4 && !strcmp(argv[1], "ids")) { printf("%d\n", queue_ids_fit((uint32_t)arg(2), arg(3)) ? 1 : 0); return 0; }
    fprintf(stderr, "usage: carve CAP max_tiles total_tiles NS max_bounces | per_path NS | ids NS slots\n");
    return 2;
}
