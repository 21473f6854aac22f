/*
 * partition_example.c -- a plain-C host that merges the 8x8 vectors of a searched and refined field into partitions of 16x16, 32x32 and
 * 64x64 samples (include/x266hip.h: "inter partition decision"), with no HIP headers:
 *
 *   frame 0: a picture (the reference); frame 1: the same picture in two pieces that move apart, the left of a slanted line by (6, -4),
 *   the right by (-5, 3)
 *     -> xConvInputFmtDev
 *     -> xSatd8x8SearchFromTilesDev, range 8                      one whole-sample vector per 8x8 block
 *     -> xSatd8x8RefineQpelFromTilesGpu                           the quarter-sample field
 *     -> xInterPartitionDecideGpu, range 1, lambda_q4 64          one vector per partition, the level per block, the price per CTU
 *     -> xMotionCompQpelGpu                                       the prediction, from the merged field as it is
 *
 * It prints the partitions per level and the summed j, and checks what the header promises of the records: the CTUs' partition counts
 * are the levels' (a block of a level-k partition is 4^-k of one), their summed distortion is the sum of the blocks' own SATDs in d_out,
 * large partitions appear where the motion is uniform, and a block whose SATD is 0 is predicted exactly.
 *
 *   usage: partition_example [width height]      (multiples of 16; default 1920 1088)      exit code 0 on success
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/x266hip.h"

#define CHECK(call) do { int rc_ = (call); if (rc_ != X266HIP_OK) { fprintf(stderr, "%s failed: %d (%s)\n", #call, rc_, xHipLastError(hip)); return 2; } } while (0)

static int lattice(int i, int j, uint32_t salt)
{
    uint32_t x = (uint32_t)i * 374761393u + (uint32_t)j * 668265263u + salt;
    x = (x ^ (x >> 13)) * 1274126177u;
    return (int)((x ^ (x >> 16)) & 255u);
}
/* value noise: a coarse field (cell 16) plus a finer one (cell 5), bilinear; smooth enough to search, without a period */
static int field(int u, int v, int cell, uint32_t salt)
{
    const int i = u / cell, j = v / cell, fu = u % cell, fv = v % cell;
    const int a = lattice(i, j, salt), b = lattice(i + 1, j, salt), c = lattice(i, j + 1, salt), d = lattice(i + 1, j + 1, salt);
    return ((a * (cell - fu) + b * fu) * (cell - fv) + (c * (cell - fu) + d * fu) * fv) / (cell * cell);
}
static uint8_t picture(int u, int v, int plane)
{
    u += 4096; v += 4096;                                                    /* the moved frame looks left of and above the origin */
    return (uint8_t)((3 * field(u, v, 16, 11u * (uint32_t)plane) + field(u, v, 5, 7u + (uint32_t)plane)) / 4);
}

int main(int argc, char **argv)
{
    const int w = argc > 2 ? atoi(argv[1]) : 1920, h = argc > 2 ? atoi(argv[2]) : 1088;
    if (w <= 0 || h <= 0 || (w & 15) || (h & 15)) { fprintf(stderr, "width and height must be multiples of 16\n"); return 2; }
    x266hip_ctx *hip = NULL;
    if (xHipCodecInit(&hip, 0) != X266HIP_OK) { fprintf(stderr, "no gfx950 device\n"); return 2; }
    const size_t npx = (size_t)w * h, nchroma = npx / 4, n = npx / 256, nb = npx / 64;
    const size_t n_ctu = (size_t)((w + 63) / 64) * (size_t)((h + 63) / 64);

    /* frame 0 is the reference; frame 1 the current frame, cur(x, y) = ref(x + mx, y + my) with (mx, my) by the side of the line */
    void *d_tiles[2];
    for (int f = 0; f < 2; f++) {
        void *d_plane[3];
        for (int p = 0; p < 3; p++) {
            const int pw = p ? w / 2 : w, ph = p ? h / 2 : h, s = p ? 2 : 1;
            uint8_t *plane = malloc(p ? nchroma : npx);
            for (int y = 0; y < ph; y++)
                for (int x = 0; x < pw; x++) {
                    const int left = s * x + s * y / 4 < 5 * w / 8;
                    const int mx = f ? (left ? 6 : -5) : 0, my = f ? (left ? -4 : 3) : 0;
                    plane[(size_t)y * pw + x] = p ? picture(x + mx / 2, y + my / 2, p) : picture(x + mx, y + my, 0);
                }
            CHECK(xHipMalloc(hip, &d_plane[p], p ? nchroma : npx));
            CHECK(xHipMemcpyH2D(hip, d_plane[p], plane, p ? nchroma : npx));
            free(plane);
        }
        CHECK(xHipMalloc(hip, &d_tiles[f], n * sizeof(x266_ref_block_t)));
        CHECK(xConvInputFmtDev(hip, (x266_ref_block_t *)d_tiles[f], d_plane[0], d_plane[1], d_plane[2], w, w, h, NULL));
        CHECK(xHipStreamSync(hip, NULL));
        for (int p = 0; p < 3; p++) xHipFree(hip, d_plane[p]);
    }
    void *d_int, *d_q, *d_out, *d_level, *d_ctu, *d_pred;
    CHECK(xHipMalloc(hip, &d_int, nb * sizeof(x266_me_result_t)));
    CHECK(xHipMalloc(hip, &d_q, nb * sizeof(x266_me_result_t)));
    CHECK(xHipMalloc(hip, &d_out, nb * sizeof(x266_me_result_t)));
    CHECK(xHipMalloc(hip, &d_level, nb));
    CHECK(xHipMalloc(hip, &d_ctu, n_ctu * sizeof(x266_part_ctu_t)));
    CHECK(xHipMalloc(hip, &d_pred, n * sizeof(x266_ref_block_t)));

    CHECK(xSatd8x8SearchFromTilesDev(hip, d_tiles[1], d_tiles[0], w, h, 8, d_int, NULL, NULL));
    CHECK(xSatd8x8RefineQpelFromTilesGpu(hip, d_tiles[1], d_tiles[0], w, h, d_int, d_q, NULL, NULL));
    x266_part_t part;
    memset(&part, 0, sizeof part);
    part.d_cur = d_tiles[1];
    part.d_ref = d_tiles[0];
    part.d_mv = d_q;
    part.d_out = d_out;
    part.d_level = d_level;
    part.d_ctu = d_ctu;
    part.d_nodes = NULL;                                                     /* the whole nodes' winners are not wanted here */
    part.width = w;
    part.height = h;
    part.range = 1;
    part.lambda_q4 = 64;
    CHECK(xInterPartitionDecideGpu(hip, &part, NULL));                       /* on the same stream, behind the refinement */
    CHECK(xMotionCompQpelGpu(hip, d_tiles[0], d_out, w, h, d_pred, NULL));   /* the merged field is an ordinary field */
    CHECK(xHipStreamSync(hip, NULL));

    x266_me_result_t *mv_q = malloc(nb * sizeof *mv_q), *mv = malloc(nb * sizeof *mv);
    uint8_t *level = malloc(nb);
    x266_part_ctu_t *ctu = malloc(n_ctu * sizeof *ctu);
    x266_ref_block_t *cur = malloc(n * sizeof *cur), *pred = malloc(n * sizeof *pred);
    CHECK(xHipMemcpyD2H(hip, mv_q, d_q, nb * sizeof *mv_q));
    CHECK(xHipMemcpyD2H(hip, mv, d_out, nb * sizeof *mv));
    CHECK(xHipMemcpyD2H(hip, level, d_level, nb));
    CHECK(xHipMemcpyD2H(hip, ctu, d_ctu, n_ctu * sizeof *ctu));
    CHECK(xHipMemcpyD2H(hip, cur, d_tiles[1], n * sizeof *cur));
    CHECK(xHipMemcpyD2H(hip, pred, d_pred, n * sizeof *pred));

    size_t blocks_at[4] = {0, 0, 0, 0}, bad_level = 0, zero = 0, zero_exact = 0;
    unsigned long long satd_in = 0, satd_out = 0, j = 0, dist = 0, bits = 0, parts = 0;
    const int bw = w / 8, tw = w / 16;
    for (size_t b = 0; b < nb; b++) {
        const int bx = (int)(b % (size_t)bw), by = (int)(b / (size_t)bw);
        satd_in += mv_q[b].cost;
        satd_out += mv[b].cost;
        if (level[b] > 3) { bad_level++; continue; }
        blocks_at[level[b]]++;
        if (mv[b].cost) continue;
        const uint8_t *c = cur[(size_t)(by >> 1) * tw + (bx >> 1)].m_Y + (by & 1) * 128 + (bx & 1) * 8;
        const uint8_t *p = pred[(size_t)(by >> 1) * tw + (bx >> 1)].m_Y + (by & 1) * 128 + (bx & 1) * 8;
        int eq = 1;
        for (int y = 0; y < 8; y++) eq &= !memcmp(c + 16 * y, p + 16 * y, 8);
        zero++;
        zero_exact += (size_t)eq;
    }
    for (size_t c = 0; c < n_ctu; c++) {
        j += ctu[c].j;
        dist += ctu[c].dist;
        bits += ctu[c].bits;
        parts += ctu[c].parts;
    }
    const size_t by_level[4] = {blocks_at[0], blocks_at[1] / 4, blocks_at[2] / 16, blocks_at[3] / 64};
    const int ok = !bad_level && blocks_at[1] % 4 == 0 && blocks_at[2] % 16 == 0 && blocks_at[3] % 64 == 0 &&
                   parts == by_level[0] + by_level[1] + by_level[2] + by_level[3] && dist == satd_out && j >= dist && zero_exact == zero &&
                   (w < 64 || h < 64 || by_level[3] > 0) && parts < nb;
    printf("{\"frame\": \"%dx%d 4:2:0\", \"blocks\": %zu, \"ctus\": %zu, \"range\": %d, \"lambda_q4\": %d, \"partitions\": [%zu, %zu, %zu, %zu], \"parts\": %llu, "
           "\"j\": %llu, \"dist\": %llu, \"bits\": %llu, \"satd_unmerged\": %llu, \"satd_merged\": %llu, \"zero_satd_blocks\": %zu, \"predicted_exactly\": %zu, "
           "\"as_expected\": %s}\n",
           w, h, nb, n_ctu, part.range, part.lambda_q4, by_level[0], by_level[1], by_level[2], by_level[3], parts, j, dist, bits, satd_in, satd_out, zero,
           zero_exact, ok ? "true" : "false");
    free(mv_q);
    free(mv);
    free(level);
    free(ctu);
    free(cur);
    free(pred);
    xHipCodecFree(hip);
    return ok ? 0 : 1;
}
