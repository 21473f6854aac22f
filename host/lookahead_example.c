/*
 * lookahead_example.c -- a plain-C host that runs three frames through the lookahead (include/x266hip.h: "lookahead"), with no HIP headers:
 *
 *   frame 0: a picture; frame 1: the same picture moved by (4, -2); frame 2: another picture
 *     -> xConvInputFmtDev -> xLaDownscaleGpu -> xLaIntraCostsGpu                 a half-size frame and its open-loop intra costs, per frame
 *     -> xSatd8x8SearchFromTilesDev on the lowres frames, against the frame before
 *     -> xLaFrameCostGpu                                                          the P decision per block and its totals
 *     -> xSceneCutFromTotals on the host                                          frame 1 continues the scene, frame 2 cuts it
 *     -> xLaPropagateGpu from the last frame of the scene back to its first      what later frames inherit from each block
 *     -> xLaTreeQpGpu                                                             the qp map of every frame
 *
 * and checks that the cut is found where it is and that frame 0, which frame 1 predicts from, gets a lower qp than frame 2.
 *
 *   usage: lookahead_example [width height [qp]]      (multiples of 32; default 1920 1088 32)      exit code 0 on success
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/x266hip.h"

#define CHECK(call) do { int rc_ = (call); if (rc_ != X266HIP_OK) { fprintf(stderr, "%s failed: %d (%s)\n", #call, rc_, xHipLastError(hip)); return 2; } } while (0)
#define FRAMES 3

static uint32_t lcg(uint32_t *s) { *s = *s * 1664525u + 1013904223u; return *s >> 8; }

int main(int argc, char **argv)
{
    const int w = argc > 2 ? atoi(argv[1]) : 1920, h = argc > 2 ? atoi(argv[2]) : 1088, qp = argc > 3 ? atoi(argv[3]) : 32;
    if (w <= 0 || h <= 0 || (w & 31) || (h & 31) || qp < 0 || qp > 51) { fprintf(stderr, "width and height must be multiples of 32, qp 0..51\n"); return 2; }
    x266hip_ctx *hip = NULL;
    if (xHipCodecInit(&hip, 0) != X266HIP_OK) { fprintf(stderr, "no gfx950 device\n"); return 2; }
    const size_t npx = (size_t)w * h, nchroma = npx / 4, n = npx / 256, n_ctu = (size_t)((w + 63) / 64) * ((h + 63) / 64);
    void *zeros = calloc(n, 8);

    /* per frame: tiles, the lowres frame, intra costs and modes, the search's records, the block records, what it received, its qp map */
    void *d_tiles[FRAMES], *d_low[FRAMES], *d_intra[FRAMES], *d_mode[FRAMES], *d_best[FRAMES], *d_block[FRAMES], *d_prop[FRAMES], *d_qp[FRAMES], *d_total;
    CHECK(xHipMalloc(hip, &d_total, 64));
    uint32_t seed = 0x266;
    for (int f = 0; f < FRAMES; f++) {
        void *d_plane[3];
        const int dx = f == 1 ? 4 : 0, dy = f == 1 ? -2 : 0, other = f == 2;
        for (int p = 0; p < 3; p++) {
            const int pw = p ? w / 2 : w, ph = p ? h / 2 : h, sx = p ? dx / 2 : dx, sy = p ? dy / 2 : dy;
            uint8_t *plane = malloc(p ? nchroma : npx);
            for (int y = 0; y < ph; y++)
                for (int x = 0; x < pw; x++) {
                    const int u = x - sx, v = y - sy;
                    const int s = other ? 128 + (int)(lcg(&seed) % 192) - 96
                                        : 128 + (int)(96.0 * (((u * 7 + v * 3 + 13 * p) % 97 + 97) % 97) / 97.0) - 48 + (((u * 31 + v * 17) % 7 + 7) % 7) - 3;
                    plane[(size_t)y * pw + x] = (uint8_t)(s < 0 ? 0 : s > 255 ? 255 : s);
                }
            CHECK(xHipMalloc(hip, &d_plane[p], p ? nchroma : npx));
            CHECK(xHipMemcpyH2D(hip, d_plane[p], plane, p ? nchroma : npx));
            free(plane);
        }
        CHECK(xHipMalloc(hip, &d_tiles[f], n * sizeof(x266_ref_block_t)));
        CHECK(xHipMalloc(hip, &d_low[f], n / 4 * sizeof(x266_ref_block_t)));
        CHECK(xHipMalloc(hip, &d_intra[f], n * 4));
        CHECK(xHipMalloc(hip, &d_mode[f], n));
        CHECK(xHipMalloc(hip, &d_best[f], n * sizeof(x266_me_result_t)));
        CHECK(xHipMalloc(hip, &d_block[f], n * sizeof(x266_la_block_t)));
        CHECK(xHipMalloc(hip, &d_prop[f], n * 8));
        CHECK(xHipMalloc(hip, &d_qp[f], n_ctu * 6));
        CHECK(xHipMemcpyH2D(hip, d_prop[f], zeros, n * 8));                /* an accumulator is zeroed once, before the first frame that refers to it */
        CHECK(xConvInputFmtDev(hip, (x266_ref_block_t *)d_tiles[f], d_plane[0], d_plane[1], d_plane[2], w, w, h, NULL));
        CHECK(xHipStreamSync(hip, NULL));
        for (int p = 0; p < 3; p++) xHipFree(hip, d_plane[p]);
    }

    /* forward: lowres frame, intra costs, search against the frame before, the P decision, the scene cut */
    int cut[FRAMES] = {1, 0, 0};                                            /* frame 0 is the key frame */
    int64_t total[FRAMES][8];
    x266_la_t la[FRAMES];
    for (int f = 0; f < FRAMES; f++) {
        memset(&la[f], 0, sizeof la[f]);
        la[f].d_src = d_tiles[f];
        la[f].d_low = d_low[f];
        la[f].d_intra = d_intra[f];
        la[f].d_mode = d_mode[f];
        la[f].d_block = d_block[f];
        la[f].d_total = d_total;
        la[f].d_prop = d_prop[f];
        la[f].d_qp = d_qp[f];
        la[f].width = w;
        la[f].height = h;
        la[f].intra_penalty = 64;
        la[f].strength_q8 = 512;
        la[f].qp = qp;
        CHECK(xLaDownscaleGpu(hip, &la[f], NULL));
        CHECK(xLaIntraCostsGpu(hip, &la[f], NULL));
        if (f > 0) {                                                        /* the lowres frame is an ordinary tiled frame of w / 2 x h / 2 */
            CHECK(xSatd8x8SearchFromTilesDev(hip, d_low[f], d_low[f - 1], w / 2, h / 2, 8, d_best[f], NULL, NULL));
            la[f].d_inter0 = d_best[f];
        }
        CHECK(xLaFrameCostGpu(hip, &la[f], NULL));                          /* frame 0 has no list: an I frame's cost */
        CHECK(xHipStreamSync(hip, NULL));
        CHECK(xHipMemcpyD2H(hip, total[f], d_total, 64));
        if (f > 0) cut[f] = xSceneCutFromTotals(total[f], 102, f, 2, 250);
        if (cut[f] < 0) { fprintf(stderr, "xSceneCutFromTotals refused frame %d\n", f); return 2; }
    }

    /* backward: every frame that continues a scene hands on to the frame it was predicted from; then the qp maps */
    for (int f = FRAMES - 1; f > 0; f--) {
        if (cut[f]) continue;
        la[f].d_prop_ref0 = d_prop[f - 1];
        CHECK(xLaPropagateGpu(hip, &la[f], NULL));
    }
    double mean_qp[FRAMES];
    uint8_t *qps = malloc(n_ctu * 6);
    for (int f = 0; f < FRAMES; f++) {
        CHECK(xLaTreeQpGpu(hip, &la[f], NULL));
        CHECK(xHipStreamSync(hip, NULL));
        CHECK(xHipMemcpyD2H(hip, qps, d_qp[f], n_ctu * 6));
        unsigned long long sum = 0;
        for (size_t i = 0; i < n_ctu * 6; i++) sum += qps[i];
        mean_qp[f] = (double)sum / (double)(n_ctu * 6);
    }
    const int ok = cut[1] == 0 && cut[2] == 1 && mean_qp[0] < mean_qp[2] && mean_qp[2] == (double)qp;
    printf("{\"frame\": \"%dx%d 4:2:0\", \"qp\": %d, \"blocks\": %zu, \"p_cost\": [%lld, %lld, %lld], \"intra_cost\": [%lld, %lld, %lld], "
           "\"list0_blocks\": [%lld, %lld, %lld], \"scene_cut\": [%d, %d, %d], \"mean_qp\": [%.2f, %.2f, %.2f], \"as_expected\": %s}\n",
           w, h, qp, n, (long long)total[0][0], (long long)total[1][0], (long long)total[2][0], (long long)total[0][1], (long long)total[1][1],
           (long long)total[2][1], (long long)total[0][3], (long long)total[1][3], (long long)total[2][3], cut[0], cut[1], cut[2], mean_qp[0], mean_qp[1],
           mean_qp[2], ok ? "true" : "false");
    free(qps);
    free(zeros);
    xHipCodecFree(hip);
    return ok ? 0 : 1;
}
