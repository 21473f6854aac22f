/*
 * entropy_stats_example.c -- a plain-C host that codes TWO 4:2:0 frames and lets the second start from the first one's statistics
 * (include/x266hip.h: xEntropyStatsLevelsGpu, xEntropyStatsSideGpu, xEntropyInitFromCounts), with no HIP headers.  Backward adaptation
 * per frame: no table crosses the wire, because the decoder derives it from what it decoded.
 *
 *   frame 1   xDct32CodeCtuTilesGpu -> levels and non-zero counts; a qp map made on the host (the side arrays: d_qp and d_nnz; all inter,
 *             all 32x32) -> xEntropyEncodeLevelsGpu + xEntropyEncodeSideGpu under the DEFAULT tables -> records and bytes to the host
 *   decoder   records and bytes into fresh device buffers -> xEntropyDecodeSideGpu, xEntropyDecodeLevelsGpu -> both statistics calls on
 *             the DECODED arrays -> xEntropyInitFromCounts: the decoder's tables
 *   encoder   both statistics calls on its own arrays -> its tables, which must be the decoder's
 *   frame 2   encoded under the encoder's tables, decoded under the decoder's; levels, counts, qp and flags compared
 *
 * It prints the bytes of frame 2 under the default and under the derived tables.  Nothing is claimed about them: the two frames are
 * synthetic and differ by a shift and fresh noise.
 *
 *   usage: entropy_stats_example [width height [qp]]      (multiples of 64; default 1920 1088 32)      exit code 0 on success
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/x266hip.h"

#define CHECK(call) do { int rc_ = (call); if (rc_ != X266HIP_OK) { fprintf(stderr, "%s failed: %d (%s)\n", #call, rc_, xHipLastError(hip)); return 2; } } while (0)

static x266hip_ctx *hip;
static uint32_t lcg(uint32_t *s) { *s = *s * 1664525u + 1013904223u; return *s >> 8; }

typedef struct frame_t {                /* what the encoder holds of a frame, in device memory */
    void *level, *nnz, *qp;
} frame_t;
typedef struct coded_t {                /* what crosses the wire, in host memory */
    x266_entropy_region_t *region;
    x266_entropy_side_ctu_t *ctu;
    uint16_t *words, *side_words;
    uint64_t n_words, n_side_words, bytes, side_bytes;
} coded_t;

static int make_frame(int w, int h, int qp, int shift, uint32_t seed, frame_t *f)
{
    const size_t npx = (size_t)w * h, nchroma = npx / 4, n_tiles = npx / 256, n_ctu = npx / 4096, n_regions = n_ctu * 6;
    void *d_plane[3], *d_tiles[2], *d_recon;
    for (int side = 0; side < 2; side++) {                                  /* the current frame, and a prediction: the picture moved and dimmed a little */
        for (int p = 0; p < 3; p++) {
            const int pw = p ? w / 2 : w, ph = p ? h / 2 : h;
            uint8_t *plane = malloc(p ? nchroma : npx);
            for (int y = 0; y < ph; y++)
                for (int x = 0; x < pw; x++) {
                    const int u = x + shift, v0 = side ? 126 + (int)(96.0 * (((u + 2) * 7 + (y + 1) * 3 + 13 * p) % 97) / 97.0) - 48
                                                       : 128 + (int)(96.0 * ((u * 7 + y * 3 + 13 * p) % 97) / 97.0) - 48 + (int)(lcg(&seed) % 7) - 3;
                    plane[(size_t)y * pw + x] = (uint8_t)(v0 < 0 ? 0 : v0 > 255 ? 255 : v0);
                }
            CHECK(xHipMalloc(hip, &d_plane[p], p ? nchroma : npx));
            CHECK(xHipMemcpyH2D(hip, d_plane[p], plane, p ? nchroma : npx));
            free(plane);
        }
        CHECK(xHipMalloc(hip, &d_tiles[side], n_tiles * sizeof(x266_ref_block_t)));
        CHECK(xConvInputFmtDev(hip, (x266_ref_block_t *)d_tiles[side], d_plane[0], d_plane[1], d_plane[2], w, w, h, NULL));
        CHECK(xHipStreamSync(hip, NULL));
        for (int p = 0; p < 3; p++) xHipFree(hip, d_plane[p]);
    }
    CHECK(xHipMalloc(hip, &f->level, n_regions * 2048));
    CHECK(xHipMalloc(hip, &f->nnz, n_regions * 4));
    CHECK(xHipMalloc(hip, &f->qp, n_regions));
    CHECK(xHipMalloc(hip, &d_recon, n_tiles * sizeof(x266_ref_block_t)));
    CHECK(xDct32CodeCtuTilesGpu(hip, d_tiles[0], d_tiles[1], w, h, NULL, qp, 171, (int16_t *)f->level, (uint32_t *)f->nnz, (x266_ref_block_t *)d_recon, NULL));
    uint8_t *map = malloc(n_regions);                                       /* a qp map that moves: the side stream's qp differences */
    for (size_t r = 0; r < n_regions; r++) {
        const int q = qp + (int)((r / 6 + (size_t)shift) % 5) - 2 + (int)(lcg(&seed) % 16 == 0);
        map[r] = (uint8_t)(q < 0 ? 0 : q > 51 ? 51 : q);
    }
    CHECK(xHipMemcpyH2D(hip, f->qp, map, n_regions));
    free(map);
    CHECK(xHipStreamSync(hip, NULL));
    xHipFree(hip, d_tiles[0]);
    xHipFree(hip, d_tiles[1]);
    xHipFree(hip, d_recon);
    return 0;
}

/* both streams of a frame under the tables (NULL: the defaults), home to the host; out == NULL: count only, the bytes returned */
static int encode_frame(const frame_t *f, size_t n_ctu, int qp, const uint16_t *init, const uint16_t *side_init, coded_t *out, uint64_t bytes[2])
{
    const size_t n_regions = 6 * n_ctu;
    void *d_region, *d_ctu, *d_total, *d_stream = NULL, *d_side = NULL;
    uint64_t total[2], side_total[2];
    CHECK(xHipMalloc(hip, &d_region, n_regions * sizeof(x266_entropy_region_t)));
    CHECK(xHipMalloc(hip, &d_ctu, n_ctu * sizeof(x266_entropy_side_ctu_t)));
    CHECK(xHipMalloc(hip, &d_total, 32));
    x266_entropy_t en = {(int16_t *)f->level, NULL, (uint32_t *)f->nnz, (x266_entropy_region_t *)d_region, NULL, (uint64_t *)d_total, init, n_regions, 0};
    x266_entropy_side_t se = {NULL, NULL, NULL, (uint8_t *)f->qp, (uint32_t *)f->nnz, (x266_entropy_side_ctu_t *)d_ctu, NULL, (uint64_t *)d_total + 2, NULL, side_init,
                              n_ctu, 0, qp, 0};
    CHECK(xEntropyEncodeLevelsGpu(hip, &en, NULL));
    CHECK(xEntropyEncodeSideGpu(hip, &se, NULL));
    CHECK(xHipStreamSync(hip, NULL));
    CHECK(xHipMemcpyD2H(hip, total, d_total, 16));
    CHECK(xHipMemcpyD2H(hip, side_total, (uint64_t *)d_total + 2, 16));
    x266_entropy_region_t *region = malloc(n_regions * sizeof *region);
    x266_entropy_side_ctu_t *ctu = malloc(n_ctu * sizeof *ctu);
    if (out) {
        CHECK(xHipMalloc(hip, &d_stream, total[0] * 2 + 16));
        CHECK(xHipMalloc(hip, &d_side, side_total[0] * 2 + 16));
        en.d_stream = (uint16_t *)d_stream;
        en.cap_words = total[0];
        se.d_stream = (uint16_t *)d_side;
        se.cap_words = side_total[0];
        CHECK(xEntropyEncodeLevelsGpu(hip, &en, NULL));
        CHECK(xEntropyEncodeSideGpu(hip, &se, NULL));
        CHECK(xHipStreamSync(hip, NULL));
    }
    CHECK(xHipMemcpyD2H(hip, region, d_region, n_regions * sizeof *region));
    CHECK(xHipMemcpyD2H(hip, ctu, d_ctu, n_ctu * sizeof *ctu));
    bytes[0] = bytes[1] = 0;
    for (size_t r = 0; r < n_regions; r++) bytes[0] += region[r].n_bytes;
    for (size_t c = 0; c < n_ctu; c++) bytes[1] += ctu[c].n_bytes;
    if (out) {
        out->region = region;
        out->ctu = ctu;
        out->n_words = total[0];
        out->n_side_words = side_total[0];
        out->bytes = bytes[0];
        out->side_bytes = bytes[1];
        out->words = malloc(total[0] * 2 + 2);
        out->side_words = malloc(side_total[0] * 2 + 2);
        if (total[0]) CHECK(xHipMemcpyD2H(hip, out->words, d_stream, total[0] * 2));
        if (side_total[0]) CHECK(xHipMemcpyD2H(hip, out->side_words, d_side, side_total[0] * 2));
        xHipFree(hip, d_stream);
        xHipFree(hip, d_side);
    } else {
        free(region);
        free(ctu);
    }
    xHipFree(hip, d_region);
    xHipFree(hip, d_ctu);
    xHipFree(hip, d_total);
    return 0;
}

typedef struct decoded_t {              /* what a decoder holds of a frame, in device memory */
    void *level, *nnz, *kind, *mode, *cls, *qp, *flag;
} decoded_t;

static int decode_frame(const coded_t *in, size_t n_ctu, int qp, const uint16_t *init, const uint16_t *side_init, decoded_t *d)
{
    const size_t n_regions = 6 * n_ctu;
    void *d_region, *d_ctu, *d_stream, *d_side;
    CHECK(xHipMalloc(hip, &d_region, n_regions * sizeof(x266_entropy_region_t)));
    CHECK(xHipMalloc(hip, &d_ctu, n_ctu * sizeof(x266_entropy_side_ctu_t)));
    CHECK(xHipMalloc(hip, &d_stream, in->n_words * 2 + 16));
    CHECK(xHipMalloc(hip, &d_side, in->n_side_words * 2 + 16));
    CHECK(xHipMemcpyH2D(hip, d_region, in->region, n_regions * sizeof(x266_entropy_region_t)));
    CHECK(xHipMemcpyH2D(hip, d_ctu, in->ctu, n_ctu * sizeof(x266_entropy_side_ctu_t)));
    if (in->n_words) CHECK(xHipMemcpyH2D(hip, d_stream, in->words, in->n_words * 2));
    if (in->n_side_words) CHECK(xHipMemcpyH2D(hip, d_side, in->side_words, in->n_side_words * 2));
    CHECK(xHipMalloc(hip, &d->level, n_regions * 2048));
    CHECK(xHipMalloc(hip, &d->nnz, n_regions * 4));
    CHECK(xHipMalloc(hip, &d->flag, n_regions * 4));
    void **bytes[4] = {&d->kind, &d->mode, &d->cls, &d->qp};
    for (int i = 0; i < 4; i++) CHECK(xHipMalloc(hip, bytes[i], n_regions));
    x266_entropy_side_t sd = {(uint8_t *)d->kind, (uint8_t *)d->mode, (uint8_t *)d->cls, (uint8_t *)d->qp, (uint32_t *)d->flag, (x266_entropy_side_ctu_t *)d_ctu,
                              (uint16_t *)d_side, NULL, NULL, side_init, n_ctu, in->n_side_words, qp, 0};
    CHECK(xEntropyDecodeSideGpu(hip, &sd, NULL));
    x266_entropy_t de = {(int16_t *)d->level, (const uint8_t *)d->cls, (uint32_t *)d->nnz, (x266_entropy_region_t *)d_region, (uint16_t *)d_stream, NULL, init, n_regions,
                         in->n_words};
    CHECK(xEntropyDecodeLevelsGpu(hip, &de, NULL));                         /* with the DECODED classes */
    CHECK(xHipStreamSync(hip, NULL));
    xHipFree(hip, d_region);
    xHipFree(hip, d_ctu);
    xHipFree(hip, d_stream);
    xHipFree(hip, d_side);
    return 0;
}

/* both statistics calls, then the two tables from the counts */
static int derive_tables(const void *level, const void *cls, const void *nnz, const void *kind, const void *mode, const void *side_cls, const void *qp_map,
                         const void *flag, size_t n_ctu, int qp, uint16_t init[X266_ENTROPY_CONTEXTS], uint16_t side_init[X266_ENTROPY_SIDE_CONTEXTS])
{
    const size_t n_regions = 6 * n_ctu;
    void *d_counts, *d_part, *d_side_part;
    uint64_t counts[2 * X266_ENTROPY_CONTEXTS], side_counts[2 * X266_ENTROPY_SIDE_CONTEXTS];
    CHECK(xHipMalloc(hip, &d_counts, sizeof counts + sizeof side_counts));
    CHECK(xHipMalloc(hip, &d_part, xEntropyStatsRows(n_regions, X266_ENTROPY_STATS_REGIONS) * 8 * X266_ENTROPY_CONTEXTS));
    CHECK(xHipMalloc(hip, &d_side_part, xEntropyStatsRows(n_ctu, X266_ENTROPY_SIDE_STATS_CTUS) * 8 * X266_ENTROPY_SIDE_CONTEXTS));
    x266_entropy_stats_t st = {(const int16_t *)level, (const uint8_t *)cls, (const uint32_t *)nnz, (uint64_t *)d_counts, (uint32_t *)d_part, n_regions};
    x266_entropy_side_stats_t ss = {(const uint8_t *)kind, (const uint8_t *)mode, (const uint8_t *)side_cls, (const uint8_t *)qp_map, (const uint32_t *)flag,
                                    (uint64_t *)d_counts + 2 * X266_ENTROPY_CONTEXTS, (uint32_t *)d_side_part, n_ctu, qp, 0};
    CHECK(xEntropyStatsLevelsGpu(hip, &st, NULL));
    CHECK(xEntropyStatsSideGpu(hip, &ss, NULL));
    CHECK(xHipStreamSync(hip, NULL));
    CHECK(xHipMemcpyD2H(hip, counts, d_counts, sizeof counts));
    CHECK(xHipMemcpyD2H(hip, side_counts, (uint64_t *)d_counts + 2 * X266_ENTROPY_CONTEXTS, sizeof side_counts));
    CHECK(xEntropyInitFromCounts(counts, X266_ENTROPY_CONTEXTS, init));
    CHECK(xEntropyInitFromCounts(side_counts, X266_ENTROPY_SIDE_CONTEXTS, side_init));
    xHipFree(hip, d_counts);
    xHipFree(hip, d_part);
    xHipFree(hip, d_side_part);
    return 0;
}

/* regions whose decoded levels, counts, qp and coded flags are the encoder's */
static int compare(const frame_t *f, const decoded_t *d, size_t n_regions, size_t equal[4])
{
    int16_t *a = malloc(n_regions * 2048), *b = malloc(n_regions * 2048);
    uint32_t *na = malloc(n_regions * 4), *nb = malloc(n_regions * 4), *flag = malloc(n_regions * 4);
    uint8_t *qa = malloc(n_regions), *qb = malloc(n_regions);
    CHECK(xHipMemcpyD2H(hip, a, f->level, n_regions * 2048));
    CHECK(xHipMemcpyD2H(hip, b, d->level, n_regions * 2048));
    CHECK(xHipMemcpyD2H(hip, na, f->nnz, n_regions * 4));
    CHECK(xHipMemcpyD2H(hip, nb, d->nnz, n_regions * 4));
    CHECK(xHipMemcpyD2H(hip, flag, d->flag, n_regions * 4));
    CHECK(xHipMemcpyD2H(hip, qa, f->qp, n_regions));
    CHECK(xHipMemcpyD2H(hip, qb, d->qp, n_regions));
    memset(equal, 0, 4 * sizeof *equal);
    for (size_t r = 0; r < n_regions; r++) {
        equal[0] += !memcmp(a + r * 1024, b + r * 1024, 2048);
        equal[1] += na[r] == nb[r];
        equal[3] += flag[r] == (na[r] != 0);
        equal[2] += na[r] ? qa[r] == qb[r] : 1;                             /* an uncoded region's qp is its predictor: the canonical form, not the map */
    }
    free(a), free(b), free(na), free(nb), free(flag), free(qa), free(qb);
    return 0;
}

int main(int argc, char **argv)
{
    const int w = argc > 2 ? atoi(argv[1]) : 1920, h = argc > 2 ? atoi(argv[2]) : 1088, qp = argc > 3 ? atoi(argv[3]) : 32;
    if (w <= 0 || h <= 0 || (w & 63) || (h & 63) || qp < 2 || qp > 48) { fprintf(stderr, "width and height must be multiples of 64, qp 2..48\n"); return 2; }
    if (xHipCodecInit(&hip, 0) != X266HIP_OK) { fprintf(stderr, "no gfx950 device\n"); return 2; }
    const size_t n_ctu = (size_t)w * h / 4096, n_regions = 6 * n_ctu;
    frame_t f1, f2;
    if (make_frame(w, h, qp, 0, 0x266, &f1) || make_frame(w, h, qp, 3, 0x1266, &f2)) return 2;

    /* frame 1 under the defaults, over the wire, decoded; tables on both sides */
    coded_t c1, c2;
    decoded_t d1, d2;
    uint64_t bytes1[2], bytes2_default[2], bytes2[2];
    if (encode_frame(&f1, n_ctu, qp, NULL, NULL, &c1, bytes1) || decode_frame(&c1, n_ctu, qp, NULL, NULL, &d1)) return 2;
    uint16_t enc_init[X266_ENTROPY_CONTEXTS], enc_side[X266_ENTROPY_SIDE_CONTEXTS], dec_init[X266_ENTROPY_CONTEXTS], dec_side[X266_ENTROPY_SIDE_CONTEXTS];
    if (derive_tables(f1.level, NULL, f1.nnz, NULL, NULL, NULL, f1.qp, f1.nnz, n_ctu, qp, enc_init, enc_side)) return 2;
    if (derive_tables(d1.level, d1.cls, d1.nnz, d1.kind, d1.mode, d1.cls, d1.qp, d1.flag, n_ctu, qp, dec_init, dec_side)) return 2;
    const int tables_equal = !memcmp(enc_init, dec_init, sizeof enc_init) && !memcmp(enc_side, dec_side, sizeof enc_side);
    int legal = 1;
    for (int i = 0; i < X266_ENTROPY_CONTEXTS; i++) legal = legal && enc_init[i] >= 31 && enc_init[i] <= 2017;
    for (int i = 0; i < X266_ENTROPY_SIDE_CONTEXTS; i++) legal = legal && enc_side[i] >= 31 && enc_side[i] <= 2017;

    /* frame 2: under the defaults to count, under the derived tables for the wire; decoded under the decoder's tables */
    if (encode_frame(&f2, n_ctu, qp, NULL, NULL, NULL, bytes2_default) || encode_frame(&f2, n_ctu, qp, enc_init, enc_side, &c2, bytes2)) return 2;
    if (decode_frame(&c2, n_ctu, qp, dec_init, dec_side, &d2)) return 2;
    size_t eq1[4], eq2[4];
    if (compare(&f1, &d1, n_regions, eq1) || compare(&f2, &d2, n_regions, eq2)) return 2;
    int bad = !tables_equal || !legal;
    for (int i = 0; i < 4; i++) bad = bad || eq1[i] != n_regions || eq2[i] != n_regions;
    printf("size 32 level table from frame 1:");
    for (int i = 75; i < 100; i++) printf(" %u", enc_init[i]);
    printf("\nside table from frame 1:");
    for (int i = 0; i < X266_ENTROPY_SIDE_CONTEXTS; i++) printf(" %u", enc_side[i]);
    printf("\n%s\n", bad ? "FAIL" : "PASS");
    printf("{\"frame\": \"%dx%d 4:2:0\", \"qp\": %d, \"ctus\": %zu, \"regions\": %zu, \"tables_equal\": %s, \"tables_legal\": %s, "
           "\"frame1_levels_equal\": %zu, \"frame1_counts_equal\": %zu, \"frame1_qp_equal\": %zu, \"frame1_flags_equal\": %zu, "
           "\"frame2_levels_equal\": %zu, \"frame2_counts_equal\": %zu, \"frame2_qp_equal\": %zu, \"frame2_flags_equal\": %zu, "
           "\"frame1_level_bytes\": %llu, \"frame1_side_bytes\": %llu, \"frame2_level_bytes_default\": %llu, \"frame2_level_bytes_derived\": %llu, "
           "\"frame2_side_bytes_default\": %llu, \"frame2_side_bytes_derived\": %llu, \"as_expected\": %s}\n",
           w, h, qp, n_ctu, n_regions, tables_equal ? "true" : "false", legal ? "true" : "false", eq1[0], eq1[1], eq1[2], eq1[3], eq2[0], eq2[1], eq2[2], eq2[3],
           (unsigned long long)bytes1[0], (unsigned long long)bytes1[1], (unsigned long long)bytes2_default[0], (unsigned long long)bytes2[0],
           (unsigned long long)bytes2_default[1], (unsigned long long)bytes2[1], bad ? "false" : "true");
    xHipCodecFree(hip);
    return bad ? 1 : 0;
}
