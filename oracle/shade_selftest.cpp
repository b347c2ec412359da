/* Stand-alone check of the oracle's shade entries for sanitizer builds (make -C oracle shade_selftest_asan): no Python, no GPU.
 * Reads a scene blob (rayn_world_desc followed by rayn_frame_params, as oracle_py.dump_scene writes them), builds the tables, records every
 * integrate call of one tile with oracle_trace_shade, runs every depth again through oracle_shade_packets and compares the outputs bit for bit.
 * Exit status 0 = equal (and, in a sanitizer build, clean). */
#include "rayn_oracle.cpp"

#include <cstdio>

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s scene.blob [tile_index]\n", argv[0]); return 2; }
    rayn_world_desc wd; rayn_frame_params p;
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(&wd, sizeof wd, 1, f) != 1 || fread(&p, sizeof p, 1, f) != 1) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    fclose(f);
    const uint32_t tile = argc > 2 ? (uint32_t)atoi(argv[2]) : 0;
    const uint32_t spp = p.samples * 4, n1 = oracle_sets_1d(p.max_bounces, p.volume_marches), n2 = oracle_sets_2d(p.max_bounces, p.volume_marches);
    std::vector<float> s1((size_t)spp * n1), s2((size_t)spp * 2 * n2), scr((size_t)p.width * p.height), fis(RAYN_FIS_TABLE_SIZE);
    oracle_build_rd_tables(spp, n1, n2, p.frame, s1.data(), s2.data());
    oracle_build_scramble(p.width, p.height, scr.data());
    oracle_build_fis_table(0, 1.5f, fis.data());
    const uint64_t cap = ((uint64_t)p.tile_w * p.tile_h * p.samples + 16) * (p.max_bounces + 2);
    std::vector<uint32_t> pk(2 * cap), lane_u(16 * cap), out_u(8 * cap), got_u(8 * cap);
    std::vector<float> lane_f(60 * cap), out_f(60 * cap), got_f(60 * cap);
    const int64_t n = oracle_trace_shade(&wd, &p, s1.data(), s2.data(), scr.data(), fis.data(), tile, cap, pk.data(), lane_u.data(), lane_f.data(), out_u.data(), out_f.data());
    if (n <= 0 || (uint64_t)n > cap) { fprintf(stderr, "oracle_trace_shade: %lld\n", (long long)n); return 1; }
    size_t bad = 0, lanes = 0;
    for (int64_t a = 0; a < n;) { /* one call per depth: the packets of a depth are contiguous */
        int64_t b = a;
        while (b < n && pk[2 * b] == pk[2 * a]) b++;
        std::vector<uint32_t> obj;
        for (int64_t k = a; k < b; k++) obj.push_back(pk[2 * k + 1]);
        const int rc = oracle_shade_packets(&wd, &p, s1.data(), s2.data(), pk[2 * a], (uint64_t)(b - a), obj.data(), &lane_u[16 * a], &lane_f[60 * a], &got_u[8 * a], &got_f[60 * a]);
        if (rc) { fprintf(stderr, "oracle_shade_packets at depth %u: %d\n", pk[2 * a], rc); return 1; }
        for (int64_t k = 8 * a; k < 8 * b; k++) bad += got_u[k] != out_u[k];
        for (int64_t k = 60 * a; k < 60 * b; k++) { uint32_t x, y; memcpy(&x, &got_f[k], 4); memcpy(&y, &out_f[k], 4); bad += x != y; }
        lanes += 4 * (size_t)(b - a);
        a = b;
    }
    printf("%lld packets, %zu lanes, %zu differing words\n", (long long)n, lanes, bad);
    return bad ? 1 : 0;
}
