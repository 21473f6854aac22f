/*
 * hier_search_example.c -- a plain-C host that runs the hierarchical motion search on two frames (include/x266hip.h: "hierarchical motion
 * search"), with no HIP headers:
 *
 *   frame 0: a picture (the reference); frame 1: the same picture moved, cur(x, y) = ref(x + 38, y - 22)
 *     -> xConvInputFmtDev -> xLaDownscaleGpu                      the two half-size frames
 *     -> xSatd8x8SearchFromTilesDev on them, range 32             one vector per 16x16 tile, in lowres samples: reaches +-64 full-resolution ones
 *     -> xSatd8x8SeededSearchGpu, seed_scale 1, centres 31, r 2   150 candidates per 8x8 block around the doubled winners and their neighbours'
 *     -> xSatd8x8RefineQpelFromTilesGpu                           the quarter-sample field
 *     -> xMotionCompQpelGpu                                       the prediction
 *
 * and checks that every block whose displaced tile lies inside the frame gets exactly (38, -22) with SATD 0 -- an even shift commutes with
 * the 2x2 mean, so the lowres search is exact there -- and that the prediction of those blocks is the current frame's samples.
 *
 *   usage: hier_search_example [width height]      (multiples of 32; default 1920 1088)      exit code 0 on success
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/x266hip.h"

#define CHECK(call) do { int rc_ = (call); if (rc_ != X266HIP_OK) { fprintf(stderr, "%s failed: %d (%s)\n", #call, rc_, xHipLastError(hip)); return 2; } } while (0)
#define MVX 38
#define MVY (-22)

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
    if (w <= 0 || h <= 0 || (w & 31) || (h & 31)) { fprintf(stderr, "width and height must be multiples of 32\n"); return 2; }
    x266hip_ctx *hip = NULL;
    if (xHipCodecInit(&hip, 0) != X266HIP_OK) { fprintf(stderr, "no gfx950 device\n"); return 2; }
    const size_t npx = (size_t)w * h, nchroma = npx / 4, n = npx / 256, nb = npx / 64;

    /* frame 0 is the reference, frame 1 the current frame: cur(x, y) = ref(x + MVX, y + MVY), chroma by half of it */
    void *d_tiles[2], *d_low[2];
    for (int f = 0; f < 2; f++) {
        void *d_plane[3];
        for (int p = 0; p < 3; p++) {
            const int pw = p ? w / 2 : w, ph = p ? h / 2 : h, sx = f ? (p ? MVX / 2 : MVX) : 0, sy = f ? (p ? MVY / 2 : MVY) : 0;
            uint8_t *plane = malloc(p ? nchroma : npx);
            for (int y = 0; y < ph; y++)
                for (int x = 0; x < pw; x++) plane[(size_t)y * pw + x] = picture(x + sx, y + sy, p);
            CHECK(xHipMalloc(hip, &d_plane[p], p ? nchroma : npx));
            CHECK(xHipMemcpyH2D(hip, d_plane[p], plane, p ? nchroma : npx));
            free(plane);
        }
        CHECK(xHipMalloc(hip, &d_tiles[f], n * sizeof(x266_ref_block_t)));
        CHECK(xHipMalloc(hip, &d_low[f], n / 4 * sizeof(x266_ref_block_t)));
        CHECK(xConvInputFmtDev(hip, (x266_ref_block_t *)d_tiles[f], d_plane[0], d_plane[1], d_plane[2], w, w, h, NULL));
        CHECK(xHipStreamSync(hip, NULL));
        for (int p = 0; p < 3; p++) xHipFree(hip, d_plane[p]);
    }
    void *d_seed, *d_int, *d_j, *d_q, *d_pred;
    CHECK(xHipMalloc(hip, &d_seed, n * sizeof(x266_me_result_t)));           /* one per 16x16 tile = per lowres 8x8 block */
    CHECK(xHipMalloc(hip, &d_int, nb * sizeof(x266_me_result_t)));
    CHECK(xHipMalloc(hip, &d_j, nb * 4));
    CHECK(xHipMalloc(hip, &d_q, nb * sizeof(x266_me_result_t)));
    CHECK(xHipMalloc(hip, &d_pred, n * sizeof(x266_ref_block_t)));

    for (int f = 0; f < 2; f++) {
        x266_la_t la;
        memset(&la, 0, sizeof la);
        la.d_src = d_tiles[f];
        la.d_low = d_low[f];
        la.width = w;
        la.height = h;
        CHECK(xLaDownscaleGpu(hip, &la, NULL));
    }
    /* the lowres frame is an ordinary tiled frame of w / 2 x h / 2 */
    CHECK(xSatd8x8SearchFromTilesDev(hip, d_low[1], d_low[0], w / 2, h / 2, 32, d_seed, NULL, NULL));
    x266_seed_t s;
    memset(&s, 0, sizeof s);
    s.d_cur = d_tiles[1];
    s.d_ref = d_tiles[0];
    s.d_seed = d_seed;
    s.d_best = d_int;
    s.d_j = d_j;
    s.width = w;
    s.height = h;
    s.seed_scale = 1;
    s.centres = 31;
    s.range = 2;
    s.lambda_q4 = 16;
    CHECK(xSatd8x8SeededSearchGpu(hip, &s, NULL));
    CHECK(xSatd8x8RefineQpelFromTilesGpu(hip, d_tiles[1], d_tiles[0], w, h, d_int, d_q, NULL, NULL));
    CHECK(xMotionCompQpelGpu(hip, d_tiles[0], d_q, w, h, d_pred, NULL));
    CHECK(xHipStreamSync(hip, NULL));

    x266_me_result_t *mv_int = malloc(nb * sizeof *mv_int), *mv_q = malloc(nb * sizeof *mv_q);
    x266_ref_block_t *cur = malloc(n * sizeof *cur), *pred = malloc(n * sizeof *pred);
    CHECK(xHipMemcpyD2H(hip, mv_int, d_int, nb * sizeof *mv_int));
    CHECK(xHipMemcpyD2H(hip, mv_q, d_q, nb * sizeof *mv_q));
    CHECK(xHipMemcpyD2H(hip, cur, d_tiles[1], n * sizeof *cur));
    CHECK(xHipMemcpyD2H(hip, pred, d_pred, n * sizeof *pred));
    size_t inside = 0, exact = 0, exact_q = 0, same = 0;
    unsigned long long satd_int = 0, satd_q = 0;
    const int bw = w / 8, tw = w / 16;
    for (size_t b = 0; b < nb; b++) {
        const int bx = (int)(b % (size_t)bw), by = (int)(b / (size_t)bw), x0 = 16 * (bx >> 1), y0 = 16 * (by >> 1);
        satd_int += mv_int[b].cost;
        satd_q += mv_q[b].cost;
        if (x0 + MVX < 0 || x0 + MVX + 15 > w - 1 || y0 + MVY < 0 || y0 + MVY + 15 > h - 1) continue;   /* the displaced tile leaves the frame */
        inside++;
        exact += mv_int[b].mvx == MVX && mv_int[b].mvy == MVY && mv_int[b].cost == 0;
        exact_q += mv_q[b].mvx == 4 * MVX && mv_q[b].mvy == 4 * MVY && mv_q[b].cost == 0;
        const uint8_t *c = cur[(size_t)(by >> 1) * tw + (bx >> 1)].m_Y + (by & 1) * 128 + (bx & 1) * 8;
        const uint8_t *p = pred[(size_t)(by >> 1) * tw + (bx >> 1)].m_Y + (by & 1) * 128 + (bx & 1) * 8;
        int eq = 1;
        for (int y = 0; y < 8; y++) eq &= !memcmp(c + 16 * y, p + 16 * y, 8);
        same += (size_t)eq;
    }
    const int ok = inside > nb / 2 && exact == inside && exact_q == inside && same == inside;
    printf("{\"frame\": \"%dx%d 4:2:0\", \"moved_by\": [%d, %d], \"blocks\": %zu, \"inside\": %zu, \"exact_integer\": %zu, \"exact_quarter\": %zu, "
           "\"predicted_exactly\": %zu, \"satd_integer\": %llu, \"satd_quarter\": %llu, \"as_expected\": %s}\n",
           w, h, MVX, MVY, nb, inside, exact, exact_q, same, satd_int, satd_q, ok ? "true" : "false");
    free(mv_int);
    free(mv_q);
    free(cur);
    free(pred);
    xHipCodecFree(hip);
    return ok ? 0 : 1;
}
