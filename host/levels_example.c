/*
 * levels_example.c -- a plain-C host that codes one 4:2:0 frame on the device and takes the levels home the compact way
 * (include/x266hip.h: xLevelsPackGpu), with no HIP headers:
 *
 *   planar Y, U, V of the current and the predicted frame (host memory)
 *     -> xConvInputFmtDev -> xDct32CodeCtuTilesGpu      the dense levels and non-zero counts of every CTU at a qp, in HBM
 *     -> xLevelsPackGpu (count only), then with a stream of exactly the size the totals name
 *     -> records, totals and stream to the host
 *     -> the walk an entropy coder does: per region the coded CGs of cg_mask, their maps, their levels, placed by xLevelScan
 *
 * and checks the walk against the dense levels, level by level.  It prints the dense and the packed byte counts.
 *
 *   usage: levels_example [width height [qp]]      (multiples of 64; default 1920 1088 32)      exit code 0 on success
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
    if (w <= 0 || h <= 0 || (w & 63) || (h & 63) || qp < 0 || qp > 51) { fprintf(stderr, "width and height must be multiples of 64, qp 0..51\n"); return 2; }
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

    /* code the frame: dense levels, 2 KiB per region */
    void *d_level, *d_nnz, *d_recon, *d_region, *d_total, *d_stream = NULL;
    CHECK(xHipMalloc(hip, &d_level, n_regions * 2048));
    CHECK(xHipMalloc(hip, &d_nnz, n_regions * 4));
    CHECK(xHipMalloc(hip, &d_recon, n_tiles * sizeof(x266_ref_block_t)));
    CHECK(xHipMalloc(hip, &d_region, n_regions * sizeof(x266_level_region_t)));
    CHECK(xHipMalloc(hip, &d_total, 16));
    CHECK(xDct32CodeCtuTilesGpu(hip, d_tiles[0], d_tiles[1], w, h, NULL, qp, 171, (int16_t *)d_level, (uint32_t *)d_nnz, (x266_ref_block_t *)d_recon, NULL));

    /* pack: once to count, once into a stream of exactly that size */
    x266_levels_t lv = {(int16_t *)d_level, NULL, (uint32_t *)d_nnz, (x266_level_region_t *)d_region, NULL, (uint64_t *)d_total, n_regions, 0};
    uint64_t total[2];
    CHECK(xLevelsPackGpu(hip, &lv, NULL));
    CHECK(xHipStreamSync(hip, NULL));
    CHECK(xHipMemcpyD2H(hip, total, d_total, 16));
    const uint64_t words = total[0];
    if (words) {
        CHECK(xHipMalloc(hip, &d_stream, words * 2));
        lv.d_stream = (uint16_t *)d_stream;
        lv.cap_words = words;
        CHECK(xLevelsPackGpu(hip, &lv, NULL));
        CHECK(xHipStreamSync(hip, NULL));
        CHECK(xHipMemcpyD2H(hip, total, d_total, 16));
    }
    x266_level_region_t *region = malloc(n_regions * sizeof *region);
    uint16_t *stream = malloc(words ? words * 2 : 2);
    int16_t *dense = malloc(n_regions * 2048), *walked = calloc(n_regions, 2048);
    CHECK(xHipMemcpyD2H(hip, region, d_region, n_regions * sizeof *region));
    if (words) CHECK(xHipMemcpyD2H(hip, stream, d_stream, words * 2));
    CHECK(xHipMemcpyD2H(hip, dense, d_level, n_regions * 2048));

    /* the coder's walk: every region here is one 32x32 block, CG bit g = scan position g */
    uint16_t pos[1024];
    if (xLevelScan(32, pos) != X266HIP_OK) { fprintf(stderr, "xLevelScan failed\n"); return 2; }
    unsigned long long nonzero = 0, sum_abs = 0, coded_cgs = 0;
    size_t bad = total[1] != n_regions || total[0] != words;
    for (size_t r = 0; r < n_regions; r++) {
        const x266_level_region_t *rec = &region[r];
        const uint16_t *map = stream + rec->offset, *level = map + __builtin_popcountll(rec->cg_mask);
        for (int g = 0; g < 64; g++) {
            if (!((rec->cg_mask >> g) & 1)) continue;
            coded_cgs++;
            for (int i = 0; i < 16; i++)
                if ((*map >> i) & 1) walked[r * 1024 + pos[g * 16 + i]] = (int16_t)*level++;
            map++;
        }
        if ((uint64_t)(level - stream) != rec->offset + rec->n_words) bad++;
        nonzero += rec->n_nz;
        sum_abs += rec->sum_abs;
    }
    if (memcmp(walked, dense, n_regions * 2048)) bad++;
    const unsigned long long dense_bytes = (unsigned long long)n_regions * 2048;
    const unsigned long long packed_bytes = (unsigned long long)words * 2 + (unsigned long long)n_regions * sizeof *region + 16;
    printf("{\"frame\": \"%dx%d 4:2:0\", \"qp\": %d, \"regions\": %zu, \"dense_bytes\": %llu, \"packed_bytes\": %llu, \"stream_words\": %llu, "
           "\"coded_cgs\": %llu, \"nonzero_levels\": %llu, \"sum_abs\": %llu, \"walk_equals_dense\": %s}\n",
           w, h, qp, n_regions, dense_bytes, packed_bytes, (unsigned long long)words, coded_cgs, nonzero, sum_abs, bad ? "false" : "true");
    xHipCodecFree(hip);
    return bad ? 1 : 0;
}
