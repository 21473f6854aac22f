/*
 * mixed_frame_example.c -- a plain-C host that codes a P-frame in which part of the picture has no counterpart in the reference
 * (include/x266hip.h: "mixed inter / intra coding of a frame"), with no HIP headers:
 *
 *   frame 0: a picture (the reference); frame 1: the same picture moved by (6, -4), with a new object -- a striped rectangle -- in it
 *     -> xConvInputFmtDev
 *     -> xSatd8x8SearchFromTilesDev, range 8 -> xSatd8x8RefineQpelFromTilesGpu     the quarter-sample field
 *     -> xMotionCompQpelGpu                                                        the inter prediction
 *     -> xDct32CodeMixedFrameGpu with every region deciding (d_kind_in NULL)       levels, counts, kinds, modes, costs, the reconstruction
 *     -> xDeblockGpu with d_kind as d_intra                                        the frame the next search would read
 *
 * It prints how many regions went intra, checks that the object's regions did and that the moved background stayed inter, and checks the
 * header's consequence (a): with every kind given as 0 the levels, counts and reconstruction are bit for bit those of
 * xDct32CodeCtuTilesGpu on the same arguments.
 *
 *   usage: mixed_frame_example [width height]      (multiples of 64, at least 256 x 256; default 1920 1088)      exit code 0 on success
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

int main(int argc, char **argv)
{
    const int w = argc > 2 ? atoi(argv[1]) : 1920, h = argc > 2 ? atoi(argv[2]) : 1088;
    if (w < 256 || h < 256 || (w & 63) || (h & 63)) { fprintf(stderr, "width and height must be multiples of 64, at least 256\n"); return 2; }
    x266hip_ctx *hip = NULL;
    if (xHipCodecInit(&hip, 0) != X266HIP_OK) { fprintf(stderr, "no gfx950 device\n"); return 2; }
    const size_t npx = (size_t)w * h, nchroma = npx / 4, n = npx / 256, nb = npx / 64;
    const int ctus_x = w / 64, ctus_y = h / 64;
    const size_t n_ctu = (size_t)ctus_x * ctus_y, n_reg = 6 * n_ctu;
    /* the object covers the CTUs [ox0, ox1) x [oy0, oy1): about a quarter of each side, in the middle */
    const int ox0 = ctus_x / 2 - (ctus_x + 7) / 8, ox1 = ctus_x / 2 + (ctus_x + 7) / 8, oy0 = ctus_y / 2 - (ctus_y + 7) / 8, oy1 = ctus_y / 2 + (ctus_y + 7) / 8;

    void *d_tiles[2];
    for (int f = 0; f < 2; f++) {
        void *d_plane[3];
        for (int p = 0; p < 3; p++) {
            const int pw = p ? w / 2 : w, ph = p ? h / 2 : h, sx = f ? (p ? MVX / 2 : MVX) : 0, sy = f ? (p ? MVY / 2 : MVY) : 0, ctu = p ? 32 : 64;
            uint8_t *plane = malloc(p ? nchroma : npx);
            for (int y = 0; y < ph; y++)
                for (int x = 0; x < pw; x++) {
                    const int in_object = f && x / ctu >= ox0 && x / ctu < ox1 && y / ctu >= oy0 && y / ctu < oy1;
                    plane[(size_t)y * pw + x] = in_object ? object(x, p) : picture(x + sx, y + sy, p);
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
    void *d_int, *d_q, *d_pred, *d_recon, *d_out, *d_level, *d_nnz, *d_kind, *d_mode, *d_cost, *d_zero, *d_level2, *d_nnz2, *d_recon2;
    CHECK(xHipMalloc(hip, &d_int, nb * sizeof(x266_me_result_t)));
    CHECK(xHipMalloc(hip, &d_q, nb * sizeof(x266_me_result_t)));
    CHECK(xHipMalloc(hip, &d_pred, n * sizeof(x266_ref_block_t)));
    CHECK(xHipMalloc(hip, &d_recon, n * sizeof(x266_ref_block_t)));
    CHECK(xHipMalloc(hip, &d_recon2, n * sizeof(x266_ref_block_t)));
    CHECK(xHipMalloc(hip, &d_out, n * sizeof(x266_ref_block_t)));
    CHECK(xHipMalloc(hip, &d_level, n_reg * 2048));
    CHECK(xHipMalloc(hip, &d_level2, n_reg * 2048));
    CHECK(xHipMalloc(hip, &d_nnz, n_reg * 4));
    CHECK(xHipMalloc(hip, &d_nnz2, n_reg * 4));
    CHECK(xHipMalloc(hip, &d_kind, n_reg));
    CHECK(xHipMalloc(hip, &d_mode, n_reg));
    CHECK(xHipMalloc(hip, &d_zero, n_reg));
    CHECK(xHipMalloc(hip, &d_cost, n_reg * 8));

    /* search, refine, predict */
    CHECK(xSatd8x8SearchFromTilesDev(hip, d_tiles[1], d_tiles[0], w, h, 8, d_int, NULL, NULL));
    CHECK(xSatd8x8RefineQpelFromTilesGpu(hip, d_tiles[1], d_tiles[0], w, h, d_int, d_q, NULL, NULL));
    CHECK(xMotionCompQpelGpu(hip, d_tiles[0], d_q, w, h, d_pred, NULL));
    /* code the frame: every region decides between the inter prediction and the 32x32 intra predictor */
    x266_mixed_t m;
    memset(&m, 0, sizeof m);
    m.d_cur = d_tiles[1];
    m.d_pred = d_pred;
    m.d_level = d_level;
    m.d_nnz = d_nnz;
    m.d_kind = d_kind;
    m.d_mode = d_mode;
    m.d_cost = d_cost;
    m.d_recon = d_recon;
    m.width = w;
    m.height = h;
    m.qp = QP;
    m.rounding = ROUNDING;
    m.intra_penalty = 64;
    CHECK(xDct32CodeMixedFrameGpu(hip, &m, NULL));
    /* deblock: the kinds are the filter's intra bytes, the counts its coded flags, the quarter-sample field its vectors */
    x266_deblock_t db;
    memset(&db, 0, sizeof db);
    db.d_intra = d_kind;
    db.d_nnz = d_nnz;
    db.d_mv = d_q;
    db.qp = QP;
    CHECK(xDeblockGpu(hip, d_recon, w, h, &db, d_out, NULL));
    CHECK(xHipStreamSync(hip, NULL));

    uint8_t *kind = malloc(n_reg), *mode = malloc(n_reg);
    uint32_t *cost = malloc(n_reg * 8);
    CHECK(xHipMemcpyD2H(hip, kind, d_kind, n_reg));
    CHECK(xHipMemcpyD2H(hip, mode, d_mode, n_reg));
    CHECK(xHipMemcpyD2H(hip, cost, d_cost, n_reg * 8));
    size_t intra = 0, object_regions = 0, object_intra = 0, background_intra = 0, consistent = 0;
    for (size_t r = 0; r < n_reg; r++) {
        const int cx = (int)(r / 6 % (size_t)ctus_x), cy = (int)(r / 6 / (size_t)ctus_x);
        /* the object's CTUs, without their first row and column: there the prediction comes from the moved background */
        const int inside = cx > ox0 && cx < ox1 && cy > oy0 && cy < oy1, border = cx >= ox0 - 1 && cx <= ox1 && cy >= oy0 - 1 && cy <= oy1;
        const int edge = cx == 0 || cy == 0 || cx == ctus_x - 1 || cy == ctus_y - 1;   /* there the displaced block leaves the reference */
        intra += kind[r];
        object_regions += (size_t)inside;
        object_intra += (size_t)(inside && kind[r]);
        background_intra += (size_t)(!border && !edge && kind[r]);
        consistent += (size_t)(kind[r] <= 1 && (kind[r] ? mode[r] < 35 && cost[2 * r + 1] + 64 < cost[2 * r] : mode[r] == 255 && cost[2 * r + 1] + 64 >= cost[2 * r]));
    }

    /* consequence (a): every kind given as 0 is the fused CTU call */
    uint8_t *zero = calloc(n_reg, 1);
    CHECK(xHipMemcpyH2D(hip, d_zero, zero, n_reg));
    m.d_kind_in = d_zero;
    m.d_level = d_level2;
    m.d_nnz = d_nnz2;
    m.d_recon = d_recon2;
    CHECK(xDct32CodeMixedFrameGpu(hip, &m, NULL));
    CHECK(xDct32CodeCtuTilesGpu(hip, d_tiles[1], d_pred, w, h, NULL, QP, ROUNDING, (int16_t *)d_level, (uint32_t *)d_nnz, (x266_ref_block_t *)d_recon, NULL));
    CHECK(xHipStreamSync(hip, NULL));
    size_t differing = 0;
    {
        void *pairs[3][2] = {{d_level, d_level2}, {d_nnz, d_nnz2}, {d_recon, d_recon2}};
        const size_t bytes[3] = {n_reg * 2048, n_reg * 4, n * sizeof(x266_ref_block_t)};
        for (int i = 0; i < 3; i++) {
            uint8_t *a = malloc(bytes[i]), *b = malloc(bytes[i]);
            CHECK(xHipMemcpyD2H(hip, a, pairs[i][0], bytes[i]));
            CHECK(xHipMemcpyD2H(hip, b, pairs[i][1], bytes[i]));
            for (size_t k = 0; k < bytes[i]; k++) differing += (size_t)((i < 2 || (k & 511) < 384) && a[k] != b[k]);   /* m_I is nobody's output */
            free(a);
            free(b);
        }
    }
    CHECK(xHipMemcpyD2H(hip, kind, d_kind, n_reg));
    size_t all_inter_kinds = 0;
    for (size_t r = 0; r < n_reg; r++) all_inter_kinds += kind[r];

    const int ok = object_regions > 0 && object_intra == object_regions && background_intra == 0 && consistent == n_reg && differing == 0 && all_inter_kinds == 0;
    printf("{\"frame\": \"%dx%d 4:2:0\", \"qp\": %d, \"regions\": %zu, \"intra\": %zu, \"object_regions\": %zu, \"object_intra\": %zu, "
           "\"background_intra\": %zu, \"consistent\": %zu, \"all_inter_differing_bytes\": %zu, \"as_expected\": %s}\n",
           w, h, QP, n_reg, intra, object_regions, object_intra, background_intra, consistent, differing, ok ? "true" : "false");
    free(kind);
    free(mode);
    free(cost);
    free(zero);
    xHipCodecFree(hip);
    return ok ? 0 : 1;
}
