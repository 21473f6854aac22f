/*
 * quality_example.c -- a plain-C host that codes one 4:2:0 frame on the device twice, once with the plain quantiser and once with
 * rate-distortion optimised quantisation, and measures each reconstruction where it lies (include/x266hip.h: xQualityStatsGpu,
 * xQualityFromTotals), with no HIP headers:
 *
 *   planar Y, U, V of the current and the predicted frame (host memory)
 *     -> xConvInputFmtDev -> xDct32FwdCtuFromTilesDev       the coefficients of every CTU, in HBM
 *     -> xQuantRegionsGpu(0) at rounding 171   |   xRdoQuantRegionsGpu at a lambda
 *     -> xQuantRegionsGpu(1) -> xDct32InvCtuToTilesDev      the reconstruction
 *     -> xQualityStatsGpu(source, reconstruction)           48 bytes per CTU and 64 bytes per frame
 *
 * and prints, for both runs, PSNR for Y, U, V and all three, SSIM for Y, U, V, and the squared error the device found beside the one
 * a host loop over both frames finds: the two must be equal, and the exit code says so.  Only the 64 bytes of totals have to reach
 * the host; the frames are copied back here for the comparison alone.
 *
 *   usage: quality_example [width height [qp [lambda]]]      (multiples of 64; default 1920 1088 32 368)      exit code 0 on success
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
    const size_t npx = (size_t)w * h, nchroma = npx / 4, n_tiles = npx / 256, n_ctu = npx / 4096, n_regions = n_ctu * 6;

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

    void *d_coef, *d_level, *d_nnz, *d_recon, *d_ctu, *d_total;
    CHECK(xHipMalloc(hip, &d_coef, n_regions * 2048));
    CHECK(xHipMalloc(hip, &d_level, n_regions * 2048));
    CHECK(xHipMalloc(hip, &d_nnz, n_regions * 4));
    CHECK(xHipMalloc(hip, &d_recon, n_tiles * sizeof(x266_ref_block_t)));
    CHECK(xHipMalloc(hip, &d_ctu, n_ctu * sizeof(x266_quality_ctu_t)));
    CHECK(xHipMalloc(hip, &d_total, 64));
    CHECK(xDct32FwdCtuFromTilesDev(hip, d_tiles[0], d_tiles[1], w, h, (int16_t *)d_coef, NULL));

    int equal = 1;
    printf("{\"frame\": \"%dx%d 4:2:0\", \"qp\": %d, \"lambda\": %d", w, h, qp, lambda);
    for (int run = 0; run < 2; run++) {
        if (run == 0) {
            CHECK(xQuantRegionsGpu(hip, 0, (const int16_t *)d_coef, (int16_t *)d_level, n_regions, NULL, NULL, qp, 171, (uint32_t *)d_nnz, NULL));
        } else {
            x266_rdoq_t rq = {(const int16_t *)d_coef, (int16_t *)d_level, NULL, NULL, (uint32_t *)d_nnz, NULL, n_regions, qp, lambda};
            CHECK(xRdoQuantRegionsGpu(hip, &rq, NULL));
        }
        CHECK(xQuantRegionsGpu(hip, 1, (const int16_t *)d_level, (int16_t *)d_level, n_regions, NULL, NULL, qp, 0, NULL, NULL));
        CHECK(xDct32InvCtuToTilesDev(hip, (const int16_t *)d_level, d_tiles[1], w, h, (x266_ref_block_t *)d_recon, NULL));
        x266_quality_t q = {(const x266_ref_block_t *)d_tiles[0], (const x266_ref_block_t *)d_recon, (x266_quality_ctu_t *)d_ctu, (int64_t *)d_total, w, h,
                            X266_QUALITY_SSE | X266_QUALITY_SSIM};
        CHECK(xQualityStatsGpu(hip, &q, NULL));                               /* on the same stream, behind the reconstruction */
        CHECK(xHipStreamSync(hip, NULL));
        int64_t total[8];
        double psnr[4], ssim[3];
        CHECK(xHipMemcpyD2H(hip, total, d_total, 64));                       /* all that has to reach the host */
        if (xQualityFromTotals(total, w, h, psnr, ssim) != X266HIP_OK) { fprintf(stderr, "xQualityFromTotals refused the device's totals\n"); return 2; }
        CHECK(xHipMemcpyD2H(hip, recon, d_recon, n_tiles * sizeof *recon));   /* for the host loop beside it only */
        unsigned long long host_sse = 0;
        for (size_t t = 0; t < n_tiles; t++)
            for (int i = 0; i < 384; i++) {                                   /* m_Y and m_C; m_I is not written */
                const int d = (int)((const uint8_t *)&recon[t])[i] - (int)((const uint8_t *)&cur[t])[i];
                host_sse += (unsigned long long)(d * d);
            }
        const unsigned long long dev_sse = (unsigned long long)(total[0] + total[1] + total[2]);
        equal &= host_sse == dev_sse;
        printf(", \"%s\": {\"psnr_y\": %.4f, \"psnr_u\": %.4f, \"psnr_v\": %.4f, \"psnr\": %.4f, \"ssim_y\": %.6f, \"ssim_u\": %.6f, \"ssim_v\": %.6f, "
               "\"sse_device\": %llu, \"sse_host\": %llu}", run ? "rdoq" : "plain", psnr[0], psnr[1], psnr[2], psnr[3], ssim[0], ssim[1], ssim[2], dev_sse, host_sse);
    }
    printf(", \"sse_equal\": %s}\n", equal ? "true" : "false");
    xHipCodecFree(hip);
    return equal ? 0 : 1;
}
