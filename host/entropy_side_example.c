/*
 * entropy_side_example.c -- a plain-C host that runs the first whole decode of the chain (include/x266hip.h: xEntropyEncodeSideGpu,
 * xEntropyDecodeSideGpu beside xEntropyEncodeLevelsGpu, xEntropyDecodeLevelsGpu), with no HIP headers:
 *
 *   frame 0: a picture (the reference); frame 1: the same picture moved by (6, -4), with a new object -- a striped CTU -- in it
 *     -> xConvInputFmtDev -> xAqStatsGpu -> xAqDecideGpu                           the qp byte of every region
 *     -> xSatd8x8SearchFromTilesDev -> xSatd8x8RefineQpelFromTilesGpu -> xMotionCompQpelGpu      the inter prediction
 *     -> xDct32CodeMixedFrameGpu under that qp map                                 levels, counts, kinds, modes
 *     -> xEntropyEncodeLevelsGpu and xEntropyEncodeSideGpu, each count only and then into a stream of exactly that size
 *     -> ONLY the records and the coded words go to the host and back into fresh device buffers
 *     -> xEntropyDecodeSideGpu                                                     kinds, modes, coded flags, classes, qp
 *     -> xEntropyDecodeLevelsGpu with the DECODED classes                          the levels
 *     -> xQuantRegionsGpu(1) with the DECODED classes and qp                       the coefficients
 *
 * and checks that levels, kinds, modes and coded flags equal the encoder's canonical ones, that the coefficients equal those from the
 * encoder's own levels and qp map, and that xEntropyEncodeSideCtu on the host gives every CTU's bytes.  The motion field would travel
 * through xEntropyEncodeMvGpu (host/entropy_motion_example.c); here the decoder side reuses the prediction.
 *
 *   usage: entropy_side_example [width height]      (multiples of 64, at least 128 x 128; default 1920 1088)      exit code 0 on success
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/x266hip.h"

#define CHECK(call) do { int rc_ = (call); if (rc_ != X266HIP_OK) { fprintf(stderr, "%s failed: %d (%s)\n", #call, rc_, xHipLastError(hip)); return 2; } } while (0)
#define MVX 6
#define MVY (-4)
#define QP 30
#define CHROMA_QP_OFFSET (-2)
#define ROUNDING 171

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
/* the new object: vertical stripes of period 8 -- nothing in the reference looks like it, and the vertical intra mode predicts it */
static uint8_t object(int x, int plane) { return (uint8_t)(((x >> (plane ? 1 : 2)) & 1) ? 208 - 16 * plane : 48 + 16 * plane); }

static unsigned canon_class(unsigned c) { c &= 15u; return (c & 3u) == 3u ? 3u : c; }

int main(int argc, char **argv)
{
    const int w = argc > 2 ? atoi(argv[1]) : 1920, h = argc > 2 ? atoi(argv[2]) : 1088;
    if (w < 128 || h < 128 || (w & 63) || (h & 63)) { fprintf(stderr, "width and height must be multiples of 64, at least 128\n"); return 2; }
    x266hip_ctx *hip = NULL;
    if (xHipCodecInit(&hip, 0) != X266HIP_OK) { fprintf(stderr, "no gfx950 device\n"); return 2; }
    const size_t npx = (size_t)w * h, nchroma = npx / 4, n = npx / 256, nb = npx / 64;
    const int ctus_x = w / 64, ctus_y = h / 64, ox = ctus_x / 2, oy = ctus_y / 2;          /* the object is the CTU (ox, oy) */
    const size_t n_ctu = (size_t)ctus_x * ctus_y, n_reg = 6 * n_ctu;

    void *d_tiles[2];
    for (int f = 0; f < 2; f++) {
        void *d_plane[3];
        for (int p = 0; p < 3; p++) {
            const int pw = p ? w / 2 : w, ph = p ? h / 2 : h, sx = f ? (p ? MVX / 2 : MVX) : 0, sy = f ? (p ? MVY / 2 : MVY) : 0, ctu = p ? 32 : 64;
            uint8_t *plane = malloc(p ? nchroma : npx);
            for (int y = 0; y < ph; y++)
                for (int x = 0; x < pw; x++) plane[(size_t)y * pw + x] = f && x / ctu == ox && y / ctu == oy ? object(x, p) : picture(x + sx, y + sy, p);
            CHECK(xHipMalloc(hip, &d_plane[p], p ? nchroma : npx));
            CHECK(xHipMemcpyH2D(hip, d_plane[p], plane, p ? nchroma : npx));
            free(plane);
        }
        CHECK(xHipMalloc(hip, &d_tiles[f], n * sizeof(x266_ref_block_t)));
        CHECK(xConvInputFmtDev(hip, (x266_ref_block_t *)d_tiles[f], d_plane[0], d_plane[1], d_plane[2], w, w, h, NULL));
        CHECK(xHipStreamSync(hip, NULL));
        for (int p = 0; p < 3; p++) xHipFree(hip, d_plane[p]);
    }
    void *d_aq_tile, *d_aq_total, *d_qp, *d_int, *d_q, *d_pred, *d_recon, *d_level, *d_nnz, *d_kind, *d_mode;
    CHECK(xHipMalloc(hip, &d_aq_tile, n * sizeof(x266_aq_tile_t)));
    CHECK(xHipMalloc(hip, &d_aq_total, 64));
    CHECK(xHipMalloc(hip, &d_qp, n_reg));
    CHECK(xHipMalloc(hip, &d_int, nb * sizeof(x266_me_result_t)));
    CHECK(xHipMalloc(hip, &d_q, nb * sizeof(x266_me_result_t)));
    CHECK(xHipMalloc(hip, &d_pred, n * sizeof(x266_ref_block_t)));
    CHECK(xHipMalloc(hip, &d_recon, n * sizeof(x266_ref_block_t)));
    CHECK(xHipMalloc(hip, &d_level, n_reg * 2048));
    CHECK(xHipMalloc(hip, &d_nnz, n_reg * 4));
    CHECK(xHipMalloc(hip, &d_kind, n_reg));
    CHECK(xHipMalloc(hip, &d_mode, n_reg));

    /* the qp map, the prediction, the coding call */
    x266_aq_t aq;
    memset(&aq, 0, sizeof aq);
    aq.d_src = d_tiles[1];
    aq.d_tile = d_aq_tile;
    aq.d_total = d_aq_total;
    aq.d_qp = d_qp;
    aq.width = w;
    aq.height = h;
    aq.mode = 1;
    aq.strength_q8 = 512;
    aq.qp = QP;
    aq.chroma_qp_offset = CHROMA_QP_OFFSET;
    CHECK(xAqStatsGpu(hip, &aq, NULL));
    CHECK(xAqDecideGpu(hip, &aq, NULL));
    CHECK(xSatd8x8SearchFromTilesDev(hip, d_tiles[1], d_tiles[0], w, h, 8, d_int, NULL, NULL));
    CHECK(xSatd8x8RefineQpelFromTilesGpu(hip, d_tiles[1], d_tiles[0], w, h, d_int, d_q, NULL, NULL));
    CHECK(xMotionCompQpelGpu(hip, d_tiles[0], d_q, w, h, d_pred, NULL));
    x266_mixed_t m;
    memset(&m, 0, sizeof m);
    m.d_cur = d_tiles[1];
    m.d_pred = d_pred;
    m.d_qp = d_qp;
    m.d_level = d_level;
    m.d_nnz = d_nnz;
    m.d_kind = d_kind;
    m.d_mode = d_mode;
    m.d_recon = d_recon;
    m.width = w;
    m.height = h;
    m.qp = QP;
    m.rounding = ROUNDING;
    m.intra_penalty = 64;
    CHECK(xDct32CodeMixedFrameGpu(hip, &m, NULL));

    /* encode levels and side information: count, then into streams of exactly the sizes the totals name */
    void *d_lrec, *d_srec, *d_ltotal, *d_stotal, *d_lstream = NULL, *d_sstream = NULL;
    CHECK(xHipMalloc(hip, &d_lrec, n_reg * sizeof(x266_entropy_region_t)));
    CHECK(xHipMalloc(hip, &d_srec, n_ctu * sizeof(x266_entropy_side_ctu_t)));
    CHECK(xHipMalloc(hip, &d_ltotal, 16));
    CHECK(xHipMalloc(hip, &d_stotal, 16));
    x266_entropy_t le = {(int16_t *)d_level, NULL, (uint32_t *)d_nnz, (x266_entropy_region_t *)d_lrec, NULL, (uint64_t *)d_ltotal, NULL, n_reg, 0};
    x266_entropy_side_t se;
    memset(&se, 0, sizeof se);
    se.d_kind = d_kind;
    se.d_mode = d_mode;
    se.d_qp = d_qp;
    se.d_nnz = d_nnz;                                                        /* d_class NULL: the mixed call codes every region 32x32 */
    se.d_coded = d_srec;
    se.d_total = d_stotal;
    se.n_ctu = n_ctu;
    se.qp = QP;
    se.chroma_qp_offset = CHROMA_QP_OFFSET;
    uint64_t ltotal[2], stotal[2];
    CHECK(xEntropyEncodeLevelsGpu(hip, &le, NULL));
    CHECK(xEntropyEncodeSideGpu(hip, &se, NULL));
    CHECK(xHipStreamSync(hip, NULL));
    CHECK(xHipMemcpyD2H(hip, ltotal, d_ltotal, 16));
    CHECK(xHipMemcpyD2H(hip, stotal, d_stotal, 16));
    const uint64_t lwords = ltotal[0], swords = stotal[0];
    if (lwords) {
        CHECK(xHipMalloc(hip, &d_lstream, lwords * 2));
        le.d_stream = d_lstream;
        le.cap_words = lwords;
        CHECK(xEntropyEncodeLevelsGpu(hip, &le, NULL));
    }
    if (swords) {
        CHECK(xHipMalloc(hip, &d_sstream, swords * 2));
        se.d_stream = d_sstream;
        se.cap_words = swords;
        CHECK(xEntropyEncodeSideGpu(hip, &se, NULL));
    }
    CHECK(xHipStreamSync(hip, NULL));
    CHECK(xHipMemcpyD2H(hip, ltotal, d_ltotal, 16));                         /* now with the count of substreams that fit: all of them */
    CHECK(xHipMemcpyD2H(hip, stotal, d_stotal, 16));

    /* what crosses: the records and the coded words, nothing else */
    x266_entropy_region_t *lrec = malloc(n_reg * sizeof *lrec);
    x266_entropy_side_ctu_t *srec = malloc(n_ctu * sizeof *srec);
    uint16_t *lstream = malloc(lwords ? lwords * 2 : 2), *sstream = malloc(swords ? swords * 2 : 2);
    CHECK(xHipMemcpyD2H(hip, lrec, d_lrec, n_reg * sizeof *lrec));
    CHECK(xHipMemcpyD2H(hip, srec, d_srec, n_ctu * sizeof *srec));
    if (lwords) CHECK(xHipMemcpyD2H(hip, lstream, d_lstream, lwords * 2));
    if (swords) CHECK(xHipMemcpyD2H(hip, sstream, d_sstream, swords * 2));
    void *r_lrec, *r_srec, *r_lstream = NULL, *r_sstream = NULL;
    CHECK(xHipMalloc(hip, &r_lrec, n_reg * sizeof *lrec));
    CHECK(xHipMalloc(hip, &r_srec, n_ctu * sizeof *srec));
    CHECK(xHipMemcpyH2D(hip, r_lrec, lrec, n_reg * sizeof *lrec));
    CHECK(xHipMemcpyH2D(hip, r_srec, srec, n_ctu * sizeof *srec));
    if (lwords) { CHECK(xHipMalloc(hip, &r_lstream, lwords * 2)); CHECK(xHipMemcpyH2D(hip, r_lstream, lstream, lwords * 2)); }
    if (swords) { CHECK(xHipMalloc(hip, &r_sstream, swords * 2)); CHECK(xHipMemcpyH2D(hip, r_sstream, sstream, swords * 2)); }

    /* the decoder: side information first, then the levels with its classes, then the coefficients with its classes and qp */
    void *r_kind, *r_mode, *r_class, *r_qp, *r_nnz, *r_status, *r_level, *r_level_nnz, *r_coef, *d_coef;
    CHECK(xHipMalloc(hip, &r_kind, n_reg));
    CHECK(xHipMalloc(hip, &r_mode, n_reg));
    CHECK(xHipMalloc(hip, &r_class, n_reg));
    CHECK(xHipMalloc(hip, &r_qp, n_reg));
    CHECK(xHipMalloc(hip, &r_nnz, n_reg * 4));
    CHECK(xHipMalloc(hip, &r_status, n_ctu));
    CHECK(xHipMalloc(hip, &r_level, n_reg * 2048));
    CHECK(xHipMalloc(hip, &r_level_nnz, n_reg * 4));
    CHECK(xHipMalloc(hip, &r_coef, n_reg * 2048));
    CHECK(xHipMalloc(hip, &d_coef, n_reg * 2048));
    x266_entropy_side_t sd;
    memset(&sd, 0, sizeof sd);
    sd.d_kind = r_kind;
    sd.d_mode = r_mode;
    sd.d_class = r_class;
    sd.d_qp = r_qp;
    sd.d_nnz = r_nnz;
    sd.d_coded = r_srec;
    sd.d_stream = r_sstream;
    sd.d_status = r_status;
    sd.n_ctu = n_ctu;
    sd.cap_words = swords;
    sd.qp = QP;
    sd.chroma_qp_offset = CHROMA_QP_OFFSET;
    CHECK(xEntropyDecodeSideGpu(hip, &sd, NULL));
    x266_entropy_t ld = {(int16_t *)r_level, (const uint8_t *)r_class, (uint32_t *)r_level_nnz, (x266_entropy_region_t *)r_lrec, (uint16_t *)r_lstream, NULL, NULL,
                         n_reg, lwords};
    CHECK(xEntropyDecodeLevelsGpu(hip, &ld, NULL));
    CHECK(xQuantRegionsGpu(hip, 1, (const int16_t *)r_level, (int16_t *)r_coef, n_reg, (const uint8_t *)r_class, (const uint8_t *)r_qp, QP, ROUNDING, NULL, NULL));
    CHECK(xQuantRegionsGpu(hip, 1, (const int16_t *)d_level, (int16_t *)d_coef, n_reg, NULL, (const uint8_t *)d_qp, QP, ROUNDING, NULL, NULL));
    CHECK(xHipStreamSync(hip, NULL));

    /* the encoder's arrays and the decoder's */
    uint8_t *kind = malloc(n_reg), *mode = malloc(n_reg), *qp = malloc(n_reg), *k2 = malloc(n_reg), *m2 = malloc(n_reg), *c2 = malloc(n_reg), *q2 = malloc(n_reg);
    uint8_t *status = malloc(n_ctu);
    uint32_t *nnz = malloc(n_reg * 4), *z2 = malloc(n_reg * 4);
    int16_t *level = malloc(n_reg * 2048), *back = malloc(n_reg * 2048), *coef = malloc(n_reg * 2048), *coef2 = malloc(n_reg * 2048);
    CHECK(xHipMemcpyD2H(hip, kind, d_kind, n_reg));
    CHECK(xHipMemcpyD2H(hip, mode, d_mode, n_reg));
    CHECK(xHipMemcpyD2H(hip, qp, d_qp, n_reg));
    CHECK(xHipMemcpyD2H(hip, nnz, d_nnz, n_reg * 4));
    CHECK(xHipMemcpyD2H(hip, k2, r_kind, n_reg));
    CHECK(xHipMemcpyD2H(hip, m2, r_mode, n_reg));
    CHECK(xHipMemcpyD2H(hip, c2, r_class, n_reg));
    CHECK(xHipMemcpyD2H(hip, q2, r_qp, n_reg));
    CHECK(xHipMemcpyD2H(hip, z2, r_nnz, n_reg * 4));
    CHECK(xHipMemcpyD2H(hip, status, r_status, n_ctu));
    CHECK(xHipMemcpyD2H(hip, level, d_level, n_reg * 2048));
    CHECK(xHipMemcpyD2H(hip, back, r_level, n_reg * 2048));
    CHECK(xHipMemcpyD2H(hip, coef, d_coef, n_reg * 2048));
    CHECK(xHipMemcpyD2H(hip, coef2, r_coef, n_reg * 2048));

    size_t levels_equal = 0, kinds_equal = 0, modes_equal = 0, flags_equal = 0, qp_equal = 0, classes_ok = 0, host_equal = 0, good_status = 0, intra = 0, coded = 0;
    size_t free_ctus = 0;
    unsigned long long side_bytes = 0, level_bytes = 0;
    for (size_t r = 0; r < n_reg; r++) {
        const size_t from = r % 6 == 5 ? r - 1 : r;                         /* one chroma kind and one chroma mode: U's */
        const unsigned K = kind[from] != 0, M = K ? (mode[from] < 34 ? mode[from] : 34u) : 255u, Z = nnz[r] != 0;
        levels_equal += !memcmp(level + r * 1024, back + r * 1024, 2048);
        kinds_equal += k2[r] == K;
        modes_equal += m2[r] == M;
        flags_equal += z2[r] == Z;
        qp_equal += !Z || q2[r] == (qp[r] < 51 ? qp[r] : 51u);              /* an uncoded region decodes to its predictor: it has no level to scale */
        classes_ok += c2[r] == canon_class(3);
        intra += K;
        coded += Z;
        level_bytes += lrec[r].n_bytes;
    }
    static uint8_t bytes[X266_ENTROPY_SIDE_MAX_BYTES];
    for (size_t c = 0; c < n_ctu; c++) {
        uint32_t bins[2];
        const int nbytes = xEntropyEncodeSideCtu(kind + 6 * c, mode + 6 * c, NULL, qp + 6 * c, nnz + 6 * c, QP, CHROMA_QP_OFFSET, NULL, bytes, sizeof bytes, bins);
        host_equal += nbytes >= 0 && (uint32_t)nbytes == srec[c].n_bytes && bins[0] == srec[c].ctx_bins && bins[1] == srec[c].bypass_bins &&
                      !memcmp(bytes, (const uint8_t *)(sstream + srec[c].offset), (size_t)nbytes);
        good_status += status[c] == 0;
        free_ctus += srec[c].n_bytes == 0;
        side_bytes += srec[c].n_bytes;
    }
    const int coef_equal = !memcmp(coef, coef2, n_reg * 2048);
    const int ok = levels_equal == n_reg && kinds_equal == n_reg && modes_equal == n_reg && flags_equal == n_reg && qp_equal == n_reg && classes_ok == n_reg &&
                   host_equal == n_ctu && good_status == n_ctu && coef_equal && intra > 0 && stotal[1] == n_ctu && ltotal[1] == n_reg;
    printf("entropy_side_example: %s\n", ok ? "PASS" : "FAIL");
    printf("{\"frame\": \"%dx%d 4:2:0\", \"qp\": %d, \"ctus\": %zu, \"regions\": %zu, \"intra_regions\": %zu, \"coded_regions\": %zu, \"level_bytes\": %llu, "
           "\"side_bytes\": %llu, \"zero_byte_ctus\": %zu, \"levels_equal\": %zu, \"kinds_equal\": %zu, \"modes_equal\": %zu, \"flags_equal\": %zu, \"qp_equal\": %zu, "
           "\"coef_equal\": %s, \"host_bytes_equal\": %zu, \"as_expected\": %s}\n",
           w, h, QP, n_ctu, n_reg, intra, coded, level_bytes, side_bytes, free_ctus, levels_equal, kinds_equal, modes_equal, flags_equal, qp_equal,
           coef_equal ? "true" : "false", host_equal, ok ? "true" : "false");
    xHipCodecFree(hip);
    return ok ? 0 : 1;
}
