/*
 * entropy_example.c -- a plain-C host that codes one 4:2:0 frame on the device and takes the levels home as range-coded bytes
 * (include/x266hip.h: xEntropyEncodeLevelsGpu, xEntropyDecodeLevelsGpu), with no HIP headers:
 *
 *   planar Y, U, V of the current and the predicted frame (host memory)
 *     -> xConvInputFmtDev -> xDct32CodeCtuTilesGpu      the dense levels and non-zero counts of every CTU at a qp, in HBM
 *     -> xLevelsBitsGpu                                 the static model's estimate of their rate
 *     -> xEntropyEncodeLevelsGpu (count only), then with a stream of exactly the size the totals name
 *     -> xEntropyDecodeLevelsGpu                        the levels again, in a second buffer
 *     -> records, stream and both level sets to the host
 *
 * and checks that decode returned the encoder's input, that xEntropyEncodeRegion on the host gives every region's bytes and bin counts, and
 * that xEntropyDecodeRegion reads them back.  It prints the coded bytes against the estimate.  The bits are the residual's alone: classes,
 * modes, qp and motion are not coded, and contexts restart at every region.
 *
 *   usage: entropy_example [width height [qp]]      (multiples of 64; default 1920 1088 32)      exit code 0 on success
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

    /* code the frame: dense levels, 2 KiB per region, and the model's estimate of them */
    void *d_level, *d_nnz, *d_recon, *d_region, *d_total, *d_stat, *d_back, *d_back_nnz, *d_stream = NULL;
    CHECK(xHipMalloc(hip, &d_level, n_regions * 2048));
    CHECK(xHipMalloc(hip, &d_back, n_regions * 2048));
    CHECK(xHipMalloc(hip, &d_nnz, n_regions * 4));
    CHECK(xHipMalloc(hip, &d_back_nnz, n_regions * 4));
    CHECK(xHipMalloc(hip, &d_recon, n_tiles * sizeof(x266_ref_block_t)));
    CHECK(xHipMalloc(hip, &d_region, n_regions * sizeof(x266_entropy_region_t)));
    CHECK(xHipMalloc(hip, &d_stat, n_regions * sizeof(x266_rdoq_region_t)));
    CHECK(xHipMalloc(hip, &d_total, 16));
    CHECK(xDct32CodeCtuTilesGpu(hip, d_tiles[0], d_tiles[1], w, h, NULL, qp, 171, (int16_t *)d_level, (uint32_t *)d_nnz, (x266_ref_block_t *)d_recon, NULL));
    x266_rdoq_t rate = {NULL, (int16_t *)d_level, NULL, NULL, (uint32_t *)d_nnz, (x266_rdoq_region_t *)d_stat, n_regions, 0, 0};
    CHECK(xLevelsBitsGpu(hip, &rate, NULL));

    /* encode: once to count, once into a stream of exactly that size; then decode into a second buffer */
    x266_entropy_t en = {(int16_t *)d_level, NULL, (uint32_t *)d_nnz, (x266_entropy_region_t *)d_region, NULL, (uint64_t *)d_total, NULL, n_regions, 0};
    uint64_t total[2];
    CHECK(xEntropyEncodeLevelsGpu(hip, &en, NULL));
    CHECK(xHipStreamSync(hip, NULL));
    CHECK(xHipMemcpyD2H(hip, total, d_total, 16));
    const uint64_t words = total[0];
    if (words) {
        CHECK(xHipMalloc(hip, &d_stream, words * 2));
        en.d_stream = (uint16_t *)d_stream;
        en.cap_words = words;
        CHECK(xEntropyEncodeLevelsGpu(hip, &en, NULL));
    }
    x266_entropy_t de = en;
    de.d_level = (int16_t *)d_back;
    de.d_nnz = (uint32_t *)d_back_nnz;
    de.d_total = NULL;
    CHECK(xEntropyDecodeLevelsGpu(hip, &de, NULL));
    CHECK(xHipStreamSync(hip, NULL));
    CHECK(xHipMemcpyD2H(hip, total, d_total, 16));

    x266_entropy_region_t *region = malloc(n_regions * sizeof *region);
    x266_rdoq_region_t *stat = malloc(n_regions * sizeof *stat);
    uint16_t *stream = malloc(words ? words * 2 : 2);
    int16_t *dense = malloc(n_regions * 2048), *back = malloc(n_regions * 2048);
    CHECK(xHipMemcpyD2H(hip, region, d_region, n_regions * sizeof *region));
    CHECK(xHipMemcpyD2H(hip, stat, d_stat, n_regions * sizeof *stat));
    if (words) CHECK(xHipMemcpyD2H(hip, stream, d_stream, words * 2));
    CHECK(xHipMemcpyD2H(hip, dense, d_level, n_regions * 2048));
    CHECK(xHipMemcpyD2H(hip, back, d_back, n_regions * 2048));

    /* the host coder, region by region: the same bytes, the same bin counts, and the same levels back */
    static uint8_t bytes[X266_ENTROPY_MAX_BYTES];
    int16_t levels[1024];
    unsigned long long coded_bytes = 0, estimate_q4 = 0, ctx_bins = 0, bypass_bins = 0, nonzero = 0;
    size_t round_trip = 0, host_equal = 0, bad = total[1] != n_regions || total[0] != words;
    for (size_t r = 0; r < n_regions; r++) {
        const x266_entropy_region_t *rec = &region[r];
        const uint8_t *sub = (const uint8_t *)(stream + rec->offset);        /* little endian words: byte j of the substream is byte j here */
        uint32_t bins[2], n_nz = 0;
        const int n = xEntropyEncodeRegion(dense + r * 1024, 3, NULL, bytes, sizeof bytes, bins);
        if (n >= 0 && (uint32_t)n == rec->n_bytes && bins[0] == rec->ctx_bins && bins[1] == rec->bypass_bins && !memcmp(bytes, sub, (size_t)n) &&
            xEntropyDecodeRegion(sub, rec->n_bytes, 3, NULL, levels, &n_nz) == 0 && n_nz == rec->n_nz && !memcmp(levels, dense + r * 1024, 2048))
            host_equal++;
        if (!memcmp(back + r * 1024, dense + r * 1024, 2048)) round_trip++;
        coded_bytes += rec->n_bytes;
        estimate_q4 += stat[r].bits;
        ctx_bins += rec->ctx_bins;
        bypass_bins += rec->bypass_bins;
        nonzero += rec->n_nz;
    }
    if (round_trip != n_regions || host_equal != n_regions) bad++;
    printf("{\"frame\": \"%dx%d 4:2:0\", \"qp\": %d, \"regions\": %zu, \"nonzero_levels\": %llu, \"stream_words\": %llu, \"coded_bytes\": %llu, \"coded_bits\": %llu, "
           "\"estimated_bits_q4\": %llu, \"coded_over_estimate\": %.4f, \"ctx_bins\": %llu, \"bypass_bins\": %llu, \"round_trip_equal\": %zu, \"host_coder_equal\": %zu, "
           "\"as_expected\": %s}\n",
           w, h, qp, n_regions, nonzero, (unsigned long long)words, coded_bytes, coded_bytes * 8, estimate_q4, estimate_q4 ? coded_bytes * 128.0 / (double)estimate_q4 : 0.0,
           ctx_bins, bypass_bins, round_trip, host_equal, bad ? "false" : "true");
    xHipCodecFree(hip);
    return bad ? 1 : 0;
}
