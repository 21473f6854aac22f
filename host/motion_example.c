/*
 * motion_example.c -- a plain-C host that takes the decided motion field off the device as the compact motion stream
 * (include/x266hip.h: "compact motion stream") and walks it the way an entropy coder and a decoder would, with no HIP headers:
 *
 *   frame 0: a picture (the reference); frame 1: the same picture in two pieces that move apart (the frames of partition_example.c)
 *     -> xConvInputFmtDev
 *     -> xSatd8x8SearchFromTilesDev, range 8                      one whole-sample vector per 8x8 block
 *     -> xSatd8x8RefineQpelFromTilesGpu                           the quarter-sample field
 *     -> xInterPartitionDecideGpu, range 1, lambda_q4 64          one vector per partition, the level per block
 *     -> xMotionPackGpu, count-only and then with a stream        32 bytes per CTU and 8 bytes per partition
 *   the host copies the records and the stream, walks every CTU with xMotionWalk, and rebuilds every vector from words 2 and 3 and
 *   xMotionPredictor over the field decoded so far -- what a decoder does -- and compares it with words 0 and 1 and with d_out
 *     -> xMotionUnpackGpu                                         the dense field again, compared with d_out and d_level
 *     -> xMotionCompQpelGpu                                       the prediction from the unpacked field
 *
 *   usage: motion_example [width height]      (multiples of 16; default 1920 1088)      exit code 0 on success
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
    const int bw = w / 8;

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
    void *d_int, *d_q, *d_out, *d_level, *d_part_ctu, *d_ctu, *d_total, *d_stream, *d_mv2, *d_level2, *d_pred;
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

    /* what crosses to the host: the records and the stream; the dense field only to compare with */
    x266_motion_ctu_t *ctu = malloc(n_ctu * sizeof *ctu);
    x266_part_ctu_t *part_ctu = malloc(n_ctu * sizeof *part_ctu);
    uint16_t *stream = malloc((size_t)words * 2);
    x266_me_result_t *out = malloc(nb * sizeof *out), *decoded = calloc(nb, sizeof *decoded), *mv2 = malloc(nb * sizeof *mv2);
    uint8_t *level = malloc(nb), *level2 = malloc(nb);
    CHECK(xHipMemcpyD2H(hip, total, d_total, sizeof total));
    CHECK(xHipMemcpyD2H(hip, ctu, d_ctu, n_ctu * sizeof *ctu));
    CHECK(xHipMemcpyD2H(hip, part_ctu, d_part_ctu, n_ctu * sizeof *part_ctu));
    CHECK(xHipMemcpyD2H(hip, stream, d_stream, (size_t)words * 2));
    CHECK(xHipMemcpyD2H(hip, out, d_out, nb * sizeof *out));
    CHECK(xHipMemcpyD2H(hip, level, d_level, nb));

    /* the walk of a host coder, and the reconstruction of a decoder: partition by partition in coding order */
    unsigned long long parts = 0, decision_parts = 0, bits = 0, decision_bits = 0, rebuilt = 0, walked_bits = 0, offset = 0;
    size_t by_level[4] = {0, 0, 0, 0};
    uint32_t max_abs = 0;
    int walk_ok = 1;
    for (size_t c = 0; c < n_ctu; c++) {
        uint8_t head[64], lvl[64];
        const int np = xMotionWalk(w, h, c, ctu[c].head_mask, head, lvl);
        walk_ok &= np > 0 && (uint32_t)np == ctu[c].parts && ctu[c].n_words == 4u * (uint32_t)np && ctu[c].offset == offset;
        if (np <= 0) break;
        const int X0 = (int)(c % (size_t)((w + 63) / 64)) * 8, Y0 = (int)(c / (size_t)((w + 63) / 64)) * 8;
        for (int j = 0; j < np; j++) {
            const unsigned i = head[j];
            const int X = X0 + (int)((i & 1u) | (i >> 1 & 2u) | (i >> 2 & 4u)), Y = Y0 + (int)((i >> 1 & 1u) | (i >> 2 & 2u) | (i >> 3 & 4u));
            const int nblk = 1 << lvl[j];
            const uint16_t *pay = stream + ctu[c].offset + 4 * (size_t)j;
            int16_t p[2];
            if (xMotionPredictor(w, h, decoded, X, Y, lvl[j], p) != X266HIP_OK) { walk_ok = 0; break; }
            const int16_t qx = (int16_t)(p[0] + (int16_t)pay[2]), qy = (int16_t)(p[1] + (int16_t)pay[3]);
            for (int y = 0; y < nblk; y++)
                for (int x = 0; x < nblk; x++) {
                    decoded[(size_t)(Y + y) * bw + (X + x)].mvx = qx;
                    decoded[(size_t)(Y + y) * bw + (X + x)].mvy = qy;
                }
            rebuilt += qx == (int16_t)pay[0] && qy == (int16_t)pay[1] && qx == out[(size_t)Y * bw + X].mvx && qy == out[(size_t)Y * bw + X].mvy &&
                       level[(size_t)Y * bw + X] == lvl[j];
            walked_bits += (unsigned)((lvl[j] > 0) + xMotionVectorBits(qx - p[0]) + xMotionVectorBits(qy - p[1]));
            by_level[lvl[j]]++;
        }
        offset += ctu[c].n_words;
        parts += ctu[c].parts;
        bits += ctu[c].bits;
        decision_parts += part_ctu[c].parts;
        decision_bits += part_ctu[c].bits;
        if (ctu[c].max_abs > max_abs) max_abs = ctu[c].max_abs;
    }

    /* the decoder's way back onto the device: records and stream in, the dense field out, and the prediction from it */
    x266_motion_t u;
    memset(&u, 0, sizeof u);
    u.d_mv = d_mv2;
    u.d_level = d_level2;
    u.d_ctu = d_ctu;
    u.d_stream = d_stream;
    u.width = w;
    u.height = h;
    u.cap_words = words;
    CHECK(xMotionUnpackGpu(hip, &u, NULL));
    CHECK(xMotionCompQpelGpu(hip, d_tiles[0], d_mv2, w, h, d_pred, NULL));
    CHECK(xHipStreamSync(hip, NULL));
    CHECK(xHipMemcpyD2H(hip, mv2, d_mv2, nb * sizeof *mv2));
    CHECK(xHipMemcpyD2H(hip, level2, d_level2, nb));
    size_t equal = 0;
    for (size_t b = 0; b < nb; b++)
        equal += mv2[b].mvx == out[b].mvx && mv2[b].mvy == out[b].mvy && mv2[b].cost == 0 && level2[b] == level[b] && decoded[b].mvx == out[b].mvx &&
                 decoded[b].mvy == out[b].mvy;

    const size_t stream_bytes = n_ctu * sizeof *ctu + (size_t)words * 2, dense_bytes = nb * 9;
    /* the whole nodes that split cost one bit each beside what the walk above added up */
    const int ok = walk_ok && total[0] == words && total[1] == n_ctu && offset == words && words == 4 * parts && parts == decision_parts && rebuilt == parts &&
                   equal == nb && bits >= walked_bits && bits - walked_bits <= 21 * n_ctu && parts < nb;
    printf("{\"frame\": \"%dx%d 4:2:0\", \"blocks\": %zu, \"ctus\": %zu, \"partitions\": [%zu, %zu, %zu, %zu], \"parts\": %llu, \"decision_parts\": %llu, "
           "\"words\": %llu, \"stream_bytes\": %zu, \"dense_bytes\": %zu, \"bits\": %llu, \"split_flags\": %llu, \"decision_bits\": %llu, \"max_abs\": %u, "
           "\"rebuilt\": %llu, \"unpacked_equal\": %zu, \"as_expected\": %s}\n",
           w, h, nb, n_ctu, by_level[0], by_level[1], by_level[2], by_level[3], parts, decision_parts, (unsigned long long)words, stream_bytes, dense_bytes, bits,
           bits - walked_bits, decision_bits, max_abs, rebuilt, equal, ok ? "true" : "false");
    free(ctu);
    free(part_ctu);
    free(stream);
    free(out);
    free(decoded);
    free(mv2);
    free(level);
    free(level2);
    xHipCodecFree(hip);
    return ok ? 0 : 1;
}
