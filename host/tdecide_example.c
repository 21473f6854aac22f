/*
 * tdecide_example.c -- a plain-C host that codes one 4:2:0 inter frame on the device with every region's transform size and type
 * chosen by rate-distortion cost (include/x266hip.h: xTransformDecideCtuTilesGpu), with no HIP headers:
 *
 *   planar Y, U, V of a reference and a current frame (host memory)
 *     -> xConvInputFmtDev                                               tiled frames, in HBM
 *     -> xSatd8x8SearchFromTilesDev -> xSatd8x8RefineQpelFromTilesGpu   quarter-sample vectors
 *     -> xMotionCompQpelGpu                                             the prediction
 *     -> xTransformDecideCtuTilesGpu                                    class byte, levels, non-zero counts, records per region
 *     -> xQuantRegionsGpu(1, d_class) -> xTransformCtuToTilesDev(d_class)   the reconstruction
 *     -> xDeblockGpu(d_class, d_nnz, vectors)                           the filtered frame
 *     -> xLevelsPackGpu(d_class)                                        the words an entropy coder would walk
 *
 * and prints the histogram of the chosen classes and, beside the same chain with every region coded as one 32x32 DCT-II
 * (xDct32FwdCtuFromTilesDev -> xRdoQuantRegionsGpu at the same lambda), the summed cost J, the estimated bits, the stream words and
 * the squared error of the reconstruction before the filter.  The estimate is the static rate model's, not a bitrate.
 *
 *   usage: tdecide_example [width height [qp [lambda]]]      (multiples of 64; default 1920 1088 32 368)      exit code 0 on success
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/x266hip.h"

#define CHECK(call) do { int rc_ = (call); if (rc_ != X266HIP_OK) { fprintf(stderr, "%s failed: %d (%s)\n", #call, rc_, xHipLastError(hip)); return 2; } } while (0)

static uint32_t hash2(uint32_t a, uint32_t b) { uint32_t x = a * 0x9E3779B1u ^ b * 0x85EBCA77u; x ^= x >> 15; x *= 0x2C1B3C6Du; x ^= x >> 13; return x; }

/* a smooth picture with, per 64x64 area, one of four textures on top: none, fine noise, sparse bright spots, a period-8 ramp */
static uint8_t picture(int x, int y, int plane, int frame)
{
    const int u = x + (frame ? 0 : 3), v = y + (frame ? 0 : -2);            /* the reference is the same picture, moved */
    int val = 128 + (int)(80.0 * (((u * 5 + v * 3 + 17 * plane) % 193) / 193.0)) - 40;
    if (frame) {                                                             /* what the prediction cannot know */
        const int cell = plane ? 32 : 64;
        const uint32_t kind = hash2((uint32_t)(x / cell), (uint32_t)(y / cell) + 977u * (uint32_t)plane) & 3u, r = hash2((uint32_t)x + 4099u * (uint32_t)plane, (uint32_t)y);
        if (kind == 1) val += (int)(r % 13u) - 6;
        else if (kind == 2) val += (r % 211u == 0) ? 70 : (int)(r % 3u) - 1;
        else if (kind == 3) val += ((x + y) % 8) * 4 - 14;
    }
    return (uint8_t)(val < 0 ? 0 : val > 255 ? 255 : val);
}

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
    const size_t npx = (size_t)w * h, nchroma = npx / 4, n_tiles = npx / 256, nb = npx / 64, n_regions = npx / 4096 * 6;

    void *d_tiles[2];                                                        /* 0: the reference, 1: the current frame */
    for (int f = 0; f < 2; f++) {
        void *d_plane[3];
        for (int p = 0; p < 3; p++) {
            const int pw = p ? w / 2 : w, ph = p ? h / 2 : h;
            uint8_t *plane = malloc(p ? nchroma : npx);
            for (int y = 0; y < ph; y++)
                for (int x = 0; x < pw; x++) plane[(size_t)y * pw + x] = picture(p ? 2 * x : x, p ? 2 * y : y, p, f);
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
    CHECK(xHipMemcpyD2H(hip, cur, d_tiles[1], n_tiles * sizeof *cur));

    void *d_int, *d_q, *d_pred, *d_class, *d_level, *d_coef, *d_nnz, *d_stat, *d_recon, *d_out, *d_region, *d_total;
    CHECK(xHipMalloc(hip, &d_int, nb * sizeof(x266_me_result_t)));
    CHECK(xHipMalloc(hip, &d_q, nb * sizeof(x266_me_result_t)));
    CHECK(xHipMalloc(hip, &d_pred, n_tiles * sizeof(x266_ref_block_t)));
    CHECK(xHipMalloc(hip, &d_class, n_regions));
    CHECK(xHipMalloc(hip, &d_level, n_regions * 2048));
    CHECK(xHipMalloc(hip, &d_coef, n_regions * 2048));
    CHECK(xHipMalloc(hip, &d_nnz, n_regions * 4));
    CHECK(xHipMalloc(hip, &d_stat, n_regions * sizeof(x266_rdoq_region_t)));
    CHECK(xHipMalloc(hip, &d_recon, n_tiles * sizeof(x266_ref_block_t)));
    CHECK(xHipMalloc(hip, &d_out, n_tiles * sizeof(x266_ref_block_t)));
    CHECK(xHipMalloc(hip, &d_region, n_regions * sizeof(x266_level_region_t)));
    CHECK(xHipMalloc(hip, &d_total, 16));
    CHECK(xHipMemcpyH2D(hip, d_recon, cur, n_tiles * sizeof *cur));          /* m_I, which no call below writes */

    /* search, refine, predict */
    CHECK(xSatd8x8SearchFromTilesDev(hip, d_tiles[1], d_tiles[0], w, h, 8, d_int, NULL, NULL));
    CHECK(xSatd8x8RefineQpelFromTilesGpu(hip, d_tiles[1], d_tiles[0], w, h, d_int, d_q, NULL, NULL));
    CHECK(xMotionCompQpelGpu(hip, d_tiles[0], d_q, w, h, d_pred, NULL));

    x266_rdoq_region_t *stat = malloc(n_regions * sizeof *stat);
    uint8_t *cls = calloc(n_regions, 1);
    unsigned long long cost[2], dist[2], bits[2], nonzero[2], words[2], sse[2], hist[16] = {0};
    for (int run = 0; run < 2; run++) {                                      /* 0: every region 32x32 DCT-II, 1: decided */
        if (run == 0) {
            x266_rdoq_t rq = {(const int16_t *)d_coef, (int16_t *)d_level, NULL, NULL, (uint32_t *)d_nnz, (x266_rdoq_region_t *)d_stat, n_regions, qp, lambda};
            CHECK(xDct32FwdCtuFromTilesDev(hip, d_tiles[1], d_pred, w, h, (int16_t *)d_coef, NULL));
            CHECK(xRdoQuantRegionsGpu(hip, &rq, NULL));
        } else {
            x266_tdecide_t td;
            memset(&td, 0, sizeof td);
            td.d_cur = d_tiles[1];
            td.d_pred = d_pred;
            td.d_class = d_class;
            td.d_level = d_level;
            td.d_nnz = d_nnz;
            td.d_stat = d_stat;
            td.width = w;
            td.height = h;
            td.qp = qp;
            td.lambda = lambda;
            td.cand_luma = td.cand_chroma = X266_TDECIDE_CLASSES;            /* whole regions only: no edge masks needed */
            for (int k = 0; k < 16; k++) td.class_bits[k] = (uint16_t)(16 * (1 + (3 - (k & 3)) + (k >> 2 ? 2 : 1)));   /* split flags + an MTS index, made up */
            CHECK(xTransformDecideCtuTilesGpu(hip, &td, NULL));
        }
        const uint8_t *k = run ? d_class : NULL;
        x266_levels_t lv = {(int16_t *)d_level, k, (uint32_t *)d_nnz, (x266_level_region_t *)d_region, NULL, (uint64_t *)d_total, n_regions, 0};
        uint64_t total[2];
        CHECK(xLevelsPackGpu(hip, &lv, NULL));                               /* count only: the words of the stream */
        CHECK(xQuantRegionsGpu(hip, 1, (const int16_t *)d_level, (int16_t *)d_coef, n_regions, k, NULL, qp, 0, NULL, NULL));
        if (run) CHECK(xTransformCtuToTilesDev(hip, (const int16_t *)d_coef, k, d_pred, w, h, (x266_ref_block_t *)d_recon, NULL));
        else     CHECK(xDct32InvCtuToTilesDev(hip, (const int16_t *)d_coef, d_pred, w, h, (x266_ref_block_t *)d_recon, NULL));
        x266_deblock_t db;
        memset(&db, 0, sizeof db);
        db.d_class = k;
        db.d_nnz = d_nnz;
        db.d_mv = d_q;
        db.qp = qp;
        CHECK(xDeblockGpu(hip, d_recon, w, h, &db, d_out, NULL));
        CHECK(xHipStreamSync(hip, NULL));
        CHECK(xHipMemcpyD2H(hip, total, d_total, 16));
        CHECK(xHipMemcpyD2H(hip, stat, d_stat, n_regions * sizeof *stat));
        CHECK(xHipMemcpyD2H(hip, recon, d_recon, n_tiles * sizeof *recon));
        if (run) CHECK(xHipMemcpyD2H(hip, cls, d_class, n_regions));
        cost[run] = dist[run] = bits[run] = nonzero[run] = sse[run] = 0;
        words[run] = total[0];
        for (size_t r = 0; r < n_regions; r++) {
            cost[run] += stat[r].dist + (unsigned long long)lambda * stat[r].bits;
            dist[run] += stat[r].dist;
            bits[run] += stat[r].bits;
            nonzero[run] += stat[r].n_nz;
            if (run) hist[cls[r] & 15]++;
        }
        for (size_t t = 0; t < n_tiles; t++)
            for (int i = 0; i < 384; i++) {                                   /* m_Y and m_C */
                const int d = (int)((const uint8_t *)&recon[t])[i] - (int)((const uint8_t *)&cur[t])[i];
                sse[run] += (unsigned long long)(d * d);
            }
    }
    printf("{\"frame\": \"%dx%d 4:2:0\", \"qp\": %d, \"lambda\": %d, \"regions\": %zu, \"class_histogram\": [", w, h, qp, lambda, n_regions);
    for (int k = 0; k < 15; k++) printf("%llu%s", hist[k], k < 14 ? ", " : "], ");
    for (int run = 0; run < 2; run++)
        printf("\"%s\": {\"sum_j_without_side_bits\": %llu, \"sum_dist\": %llu, \"estimated_bits\": %.1f, \"nonzero_levels\": %llu, \"stream_words\": %llu, \"sse\": %llu}%s",
               run ? "decided" : "all_dct32", cost[run], dist[run], bits[run] / 16.0, nonzero[run], words[run], sse[run], run ? "}\n" : ", ");
    xHipCodecFree(hip);
    return 0;
}
