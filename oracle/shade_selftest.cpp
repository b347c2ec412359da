/* Stand-alone check of the oracle's shade and ray-gen entries for sanitizer builds (make -C oracle shade_selftest_asan): no Python, no GPU.
 * Reads a scene blob (rayn_world_desc followed by rayn_frame_params, as oracle_py.dump_scene writes them), builds the tables, records every
 * integrate call of one tile with oracle_trace_shade, runs every depth again through oracle_shade_packets and compares the outputs bit for bit.
 * Then records the tile's ray-gen loop with oracle_raygen_tile - and a rectangle that is no tile of the grid - and compares every depth-0 lane the
 * integrator was handed (origin, direction, time) with the recorded ray of its (pixel, sample), bit for bit.
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
    /* the ray-gen export: the rays of this tile, then of an off-grid rectangle that shares the tile's first pixel */
    const std::vector<TileBounds> grid = build_tiles(p.width, p.height, p.tile_w, p.tile_h);
    if (tile >= grid.size()) { fprintf(stderr, "tile index out of range\n"); return 1; }
    const TileBounds b = grid[tile];
    const uint32_t ew = b.x1 - b.x0, eh = b.y1 - b.y0;
    const uint64_t np = (uint64_t)ew * eh * spp;
    std::vector<float> rf(7 * np); std::vector<uint32_t> ru(2 * np);
    const int64_t nr = oracle_raygen_tile(&wd, &p, s1.data(), s2.data(), scr.data(), fis.data(), b.x0, b.y0, b.x1, b.y1, np, rf.data(), ru.data());
    if (nr < 0 || (uint64_t)nr != np) { fprintf(stderr, "oracle_raygen_tile: %lld, expected %llu\n", (long long)nr, (unsigned long long)np); return 1; }
    size_t rbad = 0, rlanes = 0;
    for (uint64_t j = 0; j < np; j++) { /* x outer, y inner, sample innermost */
        const uint32_t s = (uint32_t)(j % spp), lp = (uint32_t)(j / spp), x = b.x0 + lp / eh, y = b.y0 + lp % eh;
        rbad += ru[2 * j] != x + y * p.width; rbad += ru[2 * j + 1] != s;
    }
    for (int64_t k = 0; k < n && pk[2 * k] == 0; k++)
        for (int i = 0; i < 4; i++) {
            const uint32_t* u = &lane_u[16 * k + 4 * i];
            if (!u[0]) continue;
            const uint64_t j = ((uint64_t)u[2] * eh + u[3]) * spp + u[1];
            if (j >= np) { rbad++; continue; }
            const float* f = &lane_f[60 * k + 15 * i];
            const float got[7] = {f[0], f[1], f[2], f[3], f[4], f[5], f[7]};
            rbad += memcmp(got, &rf[7 * j], sizeof got) != 0;
            rlanes++;
        }
    if (ew > 1 && eh > 1) { /* the same pixels through a smaller rectangle: a ray depends on its pixel and sample, not on the tile it is asked through */
        const uint64_t ns = (uint64_t)(ew - 1) * (eh - 1) * spp;
        std::vector<float> sf(7 * ns); std::vector<uint32_t> su(2 * ns);
        const int64_t m = oracle_raygen_tile(&wd, &p, s1.data(), s2.data(), scr.data(), fis.data(), b.x0, b.y0, b.x1 - 1, b.y1 - 1, ns, sf.data(), su.data());
        if (m < 0 || (uint64_t)m != ns) { fprintf(stderr, "oracle_raygen_tile (sub-rectangle): %lld\n", (long long)m); return 1; }
        for (uint64_t j = 0; j < ns; j++) {
            const uint32_t s = (uint32_t)(j % spp), lp = (uint32_t)(j / spp), lx = lp / (eh - 1), ly = lp % (eh - 1);
            const uint64_t full = ((uint64_t)lx * eh + ly) * spp + s;
            rbad += memcmp(&sf[7 * j], &rf[7 * full], 28) != 0; rbad += su[2 * j] != ru[2 * full]; rbad += su[2 * j + 1] != ru[2 * full + 1];
        }
    }
    if (oracle_raygen_tile(&wd, &p, s1.data(), s2.data(), scr.data(), fis.data(), b.x0, b.y0, p.width + 1, b.y1, np, rf.data(), ru.data()) != -1) rbad++; /* outside the film */
    printf("%llu ray-gen paths, %zu depth-0 lanes compared, %zu differing\n", (unsigned long long)np, rlanes, rbad);
    if (rlanes == 0) { fprintf(stderr, "no depth-0 lane to compare\n"); return 1; }
    return bad || rbad ? 1 : 0;
}
