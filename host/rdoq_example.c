/*
 * rdoq_example.c -- a plain-C host that codes one 4:2:0 frame on the device twice, once with the plain quantiser and once with
 * rate-distortion optimised quantisation (include/x266hip.h: xRdoQuantRegionsGpu, xLevelsBitsGpu), with no HIP headers:
 *
 *   planar Y, U, V of the current and the predicted frame (host memory)
 *     -> xConvInputFmtDev -> xDct32FwdCtuFromTilesDev       the coefficients of every CTU, in HBM
 *     -> xQuantRegionsGpu(0) at rounding 171, then xLevelsBitsGpu   |   xRdoQuantRegionsGpu at a lambda
 *     -> xQuantRegionsGpu(1) -> xDct32InvCtuToTilesDev      the reconstruction
 *     -> xLevelsPackGpu (count only)                        the words an entropy coder would walk
 *
 * and prints, for both runs, the non-zero levels, the estimated bits, the stream words and the squared error of the reconstruction
 * against the current frame.  The estimate is the static rate model's, not a bitrate.
 *
 *   usage: rdoq_example [width height [qp [lambda]]]      (multiples of 64; default 1920 1088 32 368)      exit code 0 on success
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/x266hip.h"

#define CHECK(call) do { int rc_ = (call); if (rc_ != X266HIP_OK) { fprintf(stderr, "%s failed: %d (%s)\n", #call, rc_, xHipLastError(hip)); return 2; } } while (0)

static uint32_t lcg(uint32_t *s) { *s = *s * 1664525u + 1013904223u; return *s >> 8; }

int main(int argc, char **argv)
{
    const int w = argc > 2 ? atoi(argv[1]) : 1920, h = argc > 2 ? atoi(argv[2]) : 1088, qp = argc > 3 ? atoi(argv[3]) : 32;
    const int lambda = argc > 4 ? atoi(argv[4]) : 368;
    if (w <= 0 || h <= 0 || (w & 63) || (h & 63) || qp < 0 || qp > 51 || lambda < 0 || lambda > 8192) {
        fprintf(stderr, "width and height must be multiples of 64, qp 0..51, lambda 0..8192\n");
        return 2;
    }
    x266hip_ctx *hip = NULL;
    if (xHipCodecInit(&hip, 0) != X266HIP_OK) { fprintf(stderr, "no gfx950 device\n"); return 2; }
    const size_t npx = (size_t)w * h, nchroma = npx / 4, n_tiles = npx / 256, n_regions = npx / 4096 * 6;

    /* a smooth current frame and a prediction that is the same picture moved and dimmed a little */
    void *d_plane[3], *d_tiles[2];
    uint32_t seed = 0x266;
    for (int f = 0; f < 2; f++) {
        for (int p = 0; p < 3; p++) {
            const int pw = p ? w / 2 : w, ph = p ? h / 2 : h;
            uint8_t *plane = malloc(p ? nchroma : npx);
            for (int y = 0; y < ph; y++)
                for (int x = 0; x < pw; x++) {
                    const int v = f ? 126 + (int)(96.0 * (((x + 2) * 7 + (y + 1) * 3 + 13 * p) % 97) / 97.0) - 48
                                    : 128 + (int)(96.0 * ((x * 7 + y * 3 + 13 * p) % 97) / 97.0) - 48 + (int)(lcg(&seed) % 7) - 3;
                    plane[(size_t)y * pw + x] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
                }
            CHECK(xHipMalloc(hip, &d_plane[p], p ? nchroma : npx));
            CHECK(xHipMemcpyH2D(hip, d_plane[p], plane, p ? nchroma : npx));
            free(plane);
        }
        CHECK(xHipMalloc(hip, &d_tiles[f], n_tiles * sizeof(x266_ref_block_t)));
        CHECK(xConvInputFmtDev(hip, (x266_ref_block_t *)d_tiles[f], d_plane[0], d_plane[1], d_plane[2], w, w, h, NULL));
        CHECK(xHipStreamSync(hip, NULL));
        for (int p = 0; p < 3; p++) xHipFree(hip, d_plane[p]);
    }
    x266_ref_block_t *cur = malloc(n_tiles * sizeof *cur), *recon = malloc(n_tiles * sizeof *recon);
    CHECK(xHipMemcpyD2H(hip, cur, d_tiles[0], n_tiles * sizeof *cur));

    void *d_coef, *d_level, *d_nnz, *d_stat, *d_recon, *d_region, *d_total;
    CHECK(xHipMalloc(hip, &d_coef, n_regions * 2048));
    CHECK(xHipMalloc(hip, &d_level, n_regions * 2048));
    CHECK(xHipMalloc(hip, &d_nnz, n_regions * 4));
    CHECK(xHipMalloc(hip, &d_stat, n_regions * sizeof(x266_rdoq_region_t)));
    CHECK(xHipMalloc(hip, &d_recon, n_tiles * sizeof(x266_ref_block_t)));
    CHECK(xHipMalloc(hip, &d_region, n_regions * sizeof(x266_level_region_t)));
    CHECK(xHipMalloc(hip, &d_total, 16));
    CHECK(xDct32FwdCtuFromTilesDev(hip, d_tiles[0], d_tiles[1], w, h, (int16_t *)d_coef, NULL));
    x266_rdoq_region_t *stat = malloc(n_regions * sizeof *stat);

    unsigned long long nonzero[2], bits[2], words[2], sse[2];
    for (int run = 0; run < 2; run++) {
        x266_rdoq_t rq = {(const int16_t *)d_coef, (int16_t *)d_level, NULL, NULL, (uint32_t *)d_nnz, (x266_rdoq_region_t *)d_stat, n_regions, qp, lambda};
        if (run == 0) {
            CHECK(xQuantRegionsGpu(hip, 0, (const int16_t *)d_coef, (int16_t *)d_level, n_regions, NULL, NULL, qp, 171, (uint32_t *)d_nnz, NULL));
            CHECK(xLevelsBitsGpu(hip, &rq, NULL));                           /* the same estimate for the plain quantiser's levels */
        } else {
            CHECK(xRdoQuantRegionsGpu(hip, &rq, NULL));
        }
        x266_levels_t lv = {(int16_t *)d_level, NULL, (uint32_t *)d_nnz, (x266_level_region_t *)d_region, NULL, (uint64_t *)d_total, n_regions, 0};
        uint64_t total[2];
        CHECK(xLevelsPackGpu(hip, &lv, NULL));                               /* count only: the words of the stream */
        CHECK(xQuantRegionsGpu(hip, 1, (const int16_t *)d_level, (int16_t *)d_level, n_regions, NULL, NULL, qp, 0, NULL, NULL));
        CHECK(xDct32InvCtuToTilesDev(hip, (const int16_t *)d_level, d_tiles[1], w, h, (x266_ref_block_t *)d_recon, NULL));
        CHECK(xHipStreamSync(hip, NULL));
        CHECK(xHipMemcpyD2H(hip, total, d_total, 16));
        CHECK(xHipMemcpyD2H(hip, stat, d_stat, n_regions * sizeof *stat));
        CHECK(xHipMemcpyD2H(hip, recon, d_recon, n_tiles * sizeof *recon));
        nonzero[run] = bits[run] = sse[run] = 0;
        words[run] = total[0];
        for (size_t r = 0; r < n_regions; r++) {
            nonzero[run] += stat[r].n_nz;
            bits[run] += stat[r].bits;
        }
        for (size_t t = 0; t < n_tiles; t++)
            for (int i = 0; i < 384; i++) {                                   /* m_Y and m_C; m_I is not written */
                const int d = (int)((const uint8_t *)&recon[t])[i] - (int)((const uint8_t *)&cur[t])[i];
                sse[run] += (unsigned long long)(d * d);
            }
    }
    printf("{\"frame\": \"%dx%d 4:2:0\", \"qp\": %d, \"lambda\": %d, \"regions\": %zu, "
           "\"plain\": {\"rounding\": 171, \"nonzero_levels\": %llu, \"estimated_bits\": %.1f, \"stream_words\": %llu, \"sse\": %llu}, "
           "\"rdoq\": {\"nonzero_levels\": %llu, \"estimated_bits\": %.1f, \"stream_words\": %llu, \"sse\": %llu}}\n",
           w, h, qp, lambda, n_regions, nonzero[0], bits[0] / 16.0, words[0], sse[0], nonzero[1], bits[1] / 16.0, words[1], sse[1]);
    xHipCodecFree(hip);
    return 0;
}
