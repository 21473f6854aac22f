/*
 * entropy_motion_example.c -- a plain-C host that sends the decided motion field through the entropy coder of the motion stream and back
 * (include/x266hip.h: "the entropy coder of the motion stream"), with no HIP headers:
 *
 *   the frames, the search, the refinement and the partition decision of motion_example.c
 *     -> xMotionPackGpu, count-only and then with a stream        32 bytes per CTU and 8 bytes per partition
 *     -> xEntropyEncodeMvGpu, count-only and then with a stream   32 bytes per CTU and one range-coded substream per CTU
 *   the host copies the coded records and the coded bytes out -- what a bit stream would carry -- and holds every substream against
 *   xEntropyEncodeMvCtu on the packed words; then it copies records and bytes into fresh device buffers, as a decoder would
 *     -> xEntropyDecodeMvGpu                                      pack's records and the differences, the vectors left out
 *     -> xMotionReconstructGpu                                    the dense field from the differences, compared with d_out and d_level
 *     -> xMotionCompQpelGpu                                       the prediction from it, compared with the prediction from d_out
 *
 *   usage: entropy_motion_example [width height]      (multiples of 16; default 1920 1088)      exit code 0 on success
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
    void *d_int, *d_q, *d_out, *d_level, *d_part_ctu, *d_ctu, *d_total, *d_stream, *d_mv2, *d_level2, *d_pred, *d_pred2;
    void *d_coded, *d_bytes, *d_coded2, *d_bytes2, *d_ctu2, *d_words2, *d_status;
    CHECK(xHipMalloc(hip, &d_int, nb * sizeof(x266_me_result_t)));
    CHECK(xHipMalloc(hip, &d_q, nb * sizeof(x266_me_result_t)));
    CHECK(xHipMalloc(hip, &d_out, nb * sizeof(x266_me_result_t)));
    CHECK(xHipMalloc(hip, &d_level, nb));
    CHECK(xHipMalloc(hip, &d_part_ctu, n_ctu * sizeof(x266_part_ctu_t)));
    CHECK(xHipMalloc(hip, &d_ctu, n_ctu * sizeof(x266_motion_ctu_t)));
    CHECK(xHipMalloc(hip, &d_total, 2 * sizeof(uint64_t)));
    CHECK(xHipMalloc(hip, &d_mv2, nb * sizeof(x266_me_result_t)));
    CHECK(xHipMalloc(hip, &d_level2, nb));
    CHECK(xHipMalloc(hip, &d_pred, n * sizeof(x266_ref_block_t)));
    CHECK(xHipMalloc(hip, &d_pred2, n * sizeof(x266_ref_block_t)));
    CHECK(xHipMalloc(hip, &d_coded, n_ctu * sizeof(x266_entropy_motion_ctu_t)));
    CHECK(xHipMalloc(hip, &d_coded2, n_ctu * sizeof(x266_entropy_motion_ctu_t)));
    CHECK(xHipMalloc(hip, &d_ctu2, n_ctu * sizeof(x266_motion_ctu_t)));
    CHECK(xHipMalloc(hip, &d_words2, n_ctu * 512));
    CHECK(xHipMalloc(hip, &d_status, n_ctu < 16 ? 16 : n_ctu));

    CHECK(xSatd8x8SearchFromTilesDev(hip, d_tiles[1], d_tiles[0], w, h, 8, d_int, NULL, NULL));
    CHECK(xSatd8x8RefineQpelFromTilesGpu(hip, d_tiles[1], d_tiles[0], w, h, d_int, d_q, NULL, NULL));
    x266_part_t part;
    memset(&part, 0, sizeof part);
    part.d_cur = d_tiles[1];
    part.d_ref = d_tiles[0];
    part.d_mv = d_q;
    part.d_out = d_out;
    part.d_level = d_level;
    part.d_ctu = d_part_ctu;
    part.width = w;
    part.height = h;
    part.range = 1;
    part.lambda_q4 = 64;
    CHECK(xInterPartitionDecideGpu(hip, &part, NULL));

    /* pack: first the count-only call, which sizes the stream; then the call that writes it */
    x266_motion_t m;
    memset(&m, 0, sizeof m);
    m.d_mv = d_out;
    m.d_level = d_level;
    m.d_ctu = d_ctu;
    m.d_total = d_total;
    m.width = w;
    m.height = h;
    CHECK(xMotionPackGpu(hip, &m, NULL));
    CHECK(xHipStreamSync(hip, NULL));
    uint64_t total[2];
    CHECK(xHipMemcpyD2H(hip, total, d_total, sizeof total));
    const uint64_t words = total[0];
    CHECK(xHipMalloc(hip, &d_stream, (size_t)words * 2));
    m.d_stream = d_stream;
    m.cap_words = words;
    CHECK(xMotionPackGpu(hip, &m, NULL));
    CHECK(xHipStreamSync(hip, NULL));

    /* encode: the count-only call sizes the coded stream, the second call writes it */
    x266_entropy_motion_t e;
    memset(&e, 0, sizeof e);
    e.d_ctu = d_ctu;
    e.d_words = d_stream;
    e.d_coded = d_coded;
    e.d_total = d_total;
    e.width = w;
    e.height = h;
    e.in_words = words;
    CHECK(xEntropyEncodeMvGpu(hip, &e, NULL));
    CHECK(xHipStreamSync(hip, NULL));
    CHECK(xHipMemcpyD2H(hip, total, d_total, sizeof total));
    const uint64_t coded_words = total[0];
    CHECK(xHipMalloc(hip, &d_bytes, (size_t)coded_words * 2 + 16));
    CHECK(xHipMalloc(hip, &d_bytes2, (size_t)coded_words * 2 + 16));
    e.d_stream = d_bytes;
    e.cap_words = coded_words;
    CHECK(xEntropyEncodeMvGpu(hip, &e, NULL));
    CHECK(xHipStreamSync(hip, NULL));

    /* what crosses to the host: the coded records and the coded bytes; the packed stream and the dense field only to compare with */
    x266_motion_ctu_t *ctu = malloc(n_ctu * sizeof *ctu), *ctu2 = malloc(n_ctu * sizeof *ctu2);
    x266_entropy_motion_ctu_t *coded = malloc(n_ctu * sizeof *coded);
    uint16_t *packed = malloc((size_t)words * 2 + 2), *bytes = malloc((size_t)coded_words * 2 + 2);
    x266_me_result_t *out = malloc(nb * sizeof *out), *mv2 = malloc(nb * sizeof *mv2);
    uint8_t *level = malloc(nb), *level2 = malloc(nb), *status = malloc(n_ctu);
    CHECK(xHipMemcpyD2H(hip, total, d_total, sizeof total));
    CHECK(xHipMemcpyD2H(hip, ctu, d_ctu, n_ctu * sizeof *ctu));
    CHECK(xHipMemcpyD2H(hip, coded, d_coded, n_ctu * sizeof *coded));
    if (words) CHECK(xHipMemcpyD2H(hip, packed, d_stream, (size_t)words * 2));
    if (coded_words) CHECK(xHipMemcpyD2H(hip, bytes, d_bytes, (size_t)coded_words * 2));
    CHECK(xHipMemcpyD2H(hip, out, d_out, nb * sizeof *out));
    CHECK(xHipMemcpyD2H(hip, level, d_level, nb));

    /* the device's bytes are the host coder's, CTU by CTU */
    unsigned long long bins = 0, bits = 0, coded_bytes = 0, parts = 0;
    size_t host_equal = 0;
    uint32_t longest = 0;
    for (size_t c = 0; c < n_ctu; c++) {
        uint8_t mine[X266_ENTROPY_MOTION_MAX_BYTES];
        uint32_t host_bins[2];
        const int nbytes = xEntropyEncodeMvCtu(w, h, c, ctu[c].head_mask, packed + ctu[c].offset, NULL, mine, sizeof mine, host_bins);
        host_equal += nbytes >= 0 && (uint32_t)nbytes == coded[c].n_bytes && !memcmp(mine, (const uint8_t *)(bytes + coded[c].offset), (size_t)nbytes) &&
                      host_bins[0] == coded[c].ctx_bins && host_bins[1] == coded[c].bypass_bins && coded[c].unreadable == 0 && coded[c].parts == ctu[c].parts;
        bins += coded[c].ctx_bins + coded[c].bypass_bins;
        bits += ctu[c].bits;
        coded_bytes += coded[c].n_bytes;
        parts += ctu[c].parts;
        if (coded[c].n_bytes > longest) longest = coded[c].n_bytes;
    }

    /* the decoder's side: coded records and bytes into buffers of its own, then decode, reconstruct, predict */
    CHECK(xHipMemcpyH2D(hip, d_coded2, coded, n_ctu * sizeof *coded));
    if (coded_words) CHECK(xHipMemcpyH2D(hip, d_bytes2, bytes, (size_t)coded_words * 2));
    x266_entropy_motion_t d;
    memset(&d, 0, sizeof d);
    d.d_ctu = d_ctu2;
    d.d_words = d_words2;
    d.d_coded = d_coded2;
    d.d_stream = d_bytes2;
    d.d_status = d_status;
    d.width = w;
    d.height = h;
    d.cap_words = coded_words;
    CHECK(xEntropyDecodeMvGpu(hip, &d, NULL));
    x266_motion_t u;
    memset(&u, 0, sizeof u);
    u.d_mv = d_mv2;
    u.d_level = d_level2;
    u.d_ctu = d_ctu2;
    u.d_stream = d_words2;
    u.width = w;
    u.height = h;
    u.cap_words = 256 * (uint64_t)n_ctu;
    CHECK(xMotionReconstructGpu(hip, &u, NULL));
    CHECK(xMotionCompQpelGpu(hip, d_tiles[0], d_mv2, w, h, d_pred, NULL));
    CHECK(xMotionCompQpelGpu(hip, d_tiles[0], d_out, w, h, d_pred2, NULL));
    CHECK(xHipStreamSync(hip, NULL));
    CHECK(xHipMemcpyD2H(hip, mv2, d_mv2, nb * sizeof *mv2));
    CHECK(xHipMemcpyD2H(hip, level2, d_level2, nb));
    CHECK(xHipMemcpyD2H(hip, ctu2, d_ctu2, n_ctu * sizeof *ctu2));
    CHECK(xHipMemcpyD2H(hip, status, d_status, n_ctu));
    size_t equal = 0, records_equal = 0;
    for (size_t b = 0; b < nb; b++) equal += mv2[b].mvx == out[b].mvx && mv2[b].mvy == out[b].mvy && mv2[b].cost == 0 && level2[b] == level[b];
    for (size_t c = 0; c < n_ctu; c++)
        records_equal += status[c] == 0 && ctu2[c].head_mask == ctu[c].head_mask && ctu2[c].offset == 256 * c && ctu2[c].n_words == ctu[c].n_words &&
                         ctu2[c].parts == ctu[c].parts && ctu2[c].bits == ctu[c].bits && ctu2[c].max_abs == ctu[c].max_abs;
    uint8_t *pred = malloc(n * sizeof(x266_ref_block_t)), *pred2 = malloc(n * sizeof(x266_ref_block_t));
    CHECK(xHipMemcpyD2H(hip, pred, d_pred, n * sizeof(x266_ref_block_t)));
    CHECK(xHipMemcpyD2H(hip, pred2, d_pred2, n * sizeof(x266_ref_block_t)));
    size_t pred_equal = 0;
    for (size_t t = 0; t < n; t++) pred_equal += !memcmp(pred + t * 512, pred2 + t * 512, 384);      /* m_Y and m_C; m_I is never written */

    const size_t packed_bytes = n_ctu * sizeof *ctu + (size_t)words * 2, stream_bytes = n_ctu * sizeof *coded + (size_t)coded_words * 2;
    const int ok = total[0] == coded_words && total[1] == n_ctu && host_equal == n_ctu && records_equal == n_ctu && equal == nb && pred_equal == n && bins == bits &&
                   longest <= X266_ENTROPY_MOTION_MAX_BYTES && coded_bytes > 0 && coded_bytes < packed_bytes;
    printf("{\"frame\": \"%dx%d 4:2:0\", \"blocks\": %zu, \"ctus\": %zu, \"parts\": %llu, \"packed_bytes\": %zu, \"coded_bytes\": %llu, \"stream_bytes\": %zu, "
           "\"longest\": %u, \"bits\": %llu, \"bins\": %llu, \"host_bytes_equal\": %zu, \"records_equal\": %zu, \"field_equal\": %zu, "
           "\"prediction_equal\": %s, \"as_expected\": %s}\n",
           w, h, nb, n_ctu, parts, packed_bytes, coded_bytes, stream_bytes, longest, bits, bins, host_equal, records_equal, equal, pred_equal == n ? "true" : "false",
           ok ? "true" : "false");
    free(ctu);
    free(ctu2);
    free(coded);
    free(packed);
    free(bytes);
    free(out);
    free(mv2);
    free(level);
    free(level2);
    free(status);
    free(pred);
    free(pred2);
    xHipCodecFree(hip);
    return ok ? 0 : 1;
}
