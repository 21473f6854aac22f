"""The launch options (xHipSetOption) against the entry points that read them: one table, host-only.

include/x266hip.h promises of the launch options that results never depend on them.  ROWS says, per device entry point that reads
one, which options reach its launch, what one wave takes (the "unit") and how many units the arguments make, which per-wave option
sets the length of its loop, and at which shapes it is run.  settings(row) is the list of option settings a row is swept over,
tests/test_option_cases.py holds the table against x266_amd/csrc/x266hip_abi.hip and the shapes against the conditions below (no GPU),
tests/test_gpu_options.py runs every row, shape and setting against the CPU oracle.  "autotune" is not here: test_gpu_launch_shapes.py
holds its candidate tables.

The clamp.  units_per_wave_for (x266_amd/csrc/x266_device.hpp) cuts a per-wave count to n_units / (cu_count * 40), at least 1, while
"adaptive_per_wave" is 1 (the default): on 256 CUs every launch of fewer than 20 480 units runs ONE unit per wave whatever the option
says.  So a setting that is to run a loop sets "adaptive_per_wave" to 0, and per_wave_in_force is the rule itself, for the tests to
assert with before they launch.

A shape is the keyword arguments of the row's case builder (tests/test_gpu_placement.py's for the `...Dev` rows) less the ones that
only set options there (`fixed`)."""
import collections

CU_COUNT = 256                                                              # an MI355X; the GPU tests ask the device

# every option but "autotune": the values the rows take (the bounds are kOptions': tests/test_option_cases.py)
WG_THREADS = (0, 64, 128, 192, 256)
VALUES = {
    "adaptive_per_wave": (0, 1),
    "dct32_variant": (0, 2),
    "satd_variant": (0, 1, 2, 3),
    "dct32_blocks_per_wave": (1, 2, 3, 9, 4096),
    "dct32_inv_blocks_per_wave": (1, 2, 3, 9, 4096),
    "dct32_fwdinv_blocks_per_wave": (0, 1, 2, 3, 9, 4096),
    "dct32_wg_threads": WG_THREADS,
    "satd_groups_per_wave": (0, 1, 2, 3, 9, 4096),
    "satd_wg_threads": WG_THREADS,
    "satd_lds_bytes_per_wave": (0, 16, 4096, 6144, 9216, 16384),
    "tile_tiles_per_wave": (0, 1, 2, 3, 9, 64),
    "me_tile_rows": tuple(range(9)),
}
DEFAULTS = {"adaptive_per_wave": 1, "dct32_variant": 0, "satd_variant": 0, "dct32_blocks_per_wave": 1, "dct32_inv_blocks_per_wave": 2,
            "dct32_fwdinv_blocks_per_wave": 0, "dct32_wg_threads": 0, "satd_groups_per_wave": 0, "satd_wg_threads": 0,
            "satd_lds_bytes_per_wave": 0, "tile_tiles_per_wave": 0, "me_tile_rows": 0}
PER_WAVE = ("dct32_blocks_per_wave", "dct32_inv_blocks_per_wave", "dct32_fwdinv_blocks_per_wave", "satd_groups_per_wave", "tile_tiles_per_wave")
WG_OPTIONS = ("dct32_wg_threads", "satd_wg_threads")
LOOP_LENGTHS = (2, 3, 9)                                                    # the per-wave values whose remainders the shapes cover
ADAPTIVE = "adaptive_per_wave"


# ---- the clamp ------------------------------------------------------------------------------------------------------------------
def per_wave_in_force(option_value, n_units, adaptive, cu_count):
    """units_per_wave_for of x266_device.hpp: the units one wave loops over when the LaunchCfg holds `option_value`"""
    u = max(int(option_value), 1)
    if adaptive:
        cap = n_units // (cu_count * 40)
        if cap < u:
            u = max(cap, 1)
    return u


SATD_DMA_MIN_BLOCKS = 3 << 20                                               # kSatdDmaMinBlocks


def satd_default_groups(satd_variant, n_blocks, frame_lanes=False):
    """what the SATD launchers make of "satd_groups_per_wave" 0 before the clamp: 2 for the staged body and the frame lanes, 4 for the
    LDS-DMA body (launch_satd8x8, launch_frame_lanes)"""
    dma = not frame_lanes and (satd_variant == 3 or (satd_variant == 0 and n_blocks >= SATD_DMA_MIN_BLOCKS))
    return 4 if dma else 2


# ---- the table ----------------------------------------------------------------------------------------------------------------------
# entry: the C entry point.  options: the options that reach its launch.  unit / units(shape): what one wave takes, and how many there
# are.  loop: the per-wave option of its loop (None: one unit per wave, or a fixed count).  zero(setting, shape): what the value 0 of
# that option stands for.  live(shape): the shapes whose launch has the loop (a row may hold shapes that take another kernel).
# wg: the workgroup-size option (None: a fixed workgroup).  wg_fixed: waves per workgroup when there is no such option.  base: options
# every setting of the row holds.  unused: options the call's configuration carries and its launch ignores (swept all the same: the
# promise covers them).  frame: the units are a raster, grid(shape) = (rows, columns).  fives: five waves per CTU.
Row = collections.namedtuple("Row", "name entry options unused unit units shapes fixed loop zero live wg wg_fixed base frame fives pairs builder")
ROWS = collections.OrderedDict()


def _row(name, entry, options, unit, units, shapes, fixed=None, loop=None, zero=None, live=None, wg=None, wg_fixed=1, base=None, frame=None,
         fives=False, pairs=True, builder=None, unused=()):
    assert name not in ROWS and (loop is None or loop in options) and (wg is None or wg in options) and not set(unused) & set(options)
    ROWS[name] = Row(name, entry, tuple(options), tuple(unused), unit, units, list(shapes), dict(fixed or {}), loop, zero or (lambda setting, shape: 1),
                     live or (lambda shape: True), wg, wg_fixed, dict(base or {}), frame, fives, pairs, builder or entry)


def _n(shape):
    return shape["n"]


# unit counts of the batch rows: 1; remainders 1 and p - 1 of 2, 3 and 9; fewer than p; 24 = 2 * 3 * 4 and 108 = 9 * 12 waves of one unit
BATCH_UNITS = (1, 2, 3, 4, 5, 7, 8, 10, 13, 17, 19, 24, 28, 37, 108)
DCT = "dct32_wg_threads"

_row("xDct32FwdBatchDev", "xDct32FwdBatchDev", ("dct32_variant", DCT, "dct32_blocks_per_wave", ADAPTIVE), "32x32 block", _n,
     [dict(n=n) for n in BATCH_UNITS], fixed=dict(opt=(0, 0, 1)), loop="dct32_blocks_per_wave", wg=DCT)
_row("xDct32InvBatchDev", "xDct32InvBatchDev", (DCT, "dct32_inv_blocks_per_wave", ADAPTIVE), "32x32 block", _n,
     [dict(n=n) for n in BATCH_UNITS], fixed=dict(bpw=2, wg=0), loop="dct32_inv_blocks_per_wave", wg=DCT)
for _coef in (True, False):                                                 # 0 = automatic: 2 blocks per wave, 8 without d_coef
    _row("xDct32FwdInvBatchDev-%s" % ("coef" if _coef else "recon"), "xDct32FwdInvBatchDev", (DCT, "dct32_fwdinv_blocks_per_wave", ADAPTIVE),
         "32x32 block", _n, [dict(n=n, coef=_coef) for n in BATCH_UNITS], fixed=dict(bpw=0, wg=0), loop="dct32_fwdinv_blocks_per_wave",
         zero=(lambda setting, shape: 2 if shape["coef"] else 8), wg=DCT)


def _groups(n_blocks):
    return (n_blocks + 31) // 32


def _ragged(groups):
    """blocks of `groups` 32-block groups, the last one short unless the count is a multiple of three"""
    return 32 * groups - 7 * (groups % 3)


SATD = ("satd_variant", "satd_groups_per_wave", "satd_wg_threads", "satd_lds_bytes_per_wave", ADAPTIVE)
# the frame lanes take the SATD configuration and use its run length alone: two-wave workgroups, the staged body
_row("xDct32SatdFrameDev", "xDct32SatdFrameDev", ("satd_groups_per_wave", ADAPTIVE), "32-block SATD group", lambda s: _groups(s["n"][1]),
     [dict(n=(1 + g % 4, _ragged(g))) for g in BATCH_UNITS], fixed=dict(satd_variant=0), loop="satd_groups_per_wave",
     zero=lambda setting, shape: 2, wg_fixed=2, unused=("satd_variant", "satd_wg_threads", "satd_lds_bytes_per_wave"))
# the batch: the staged body (variants 0 and 1 at these sizes), and the LDS-DMA body forced onto the same shapes; the butterfly
# (variant 2) takes 64 blocks per wave whatever the run length says
_row("xSatd8x8BatchDev-staged", "xSatd8x8BatchDev", SATD, "32-block SATD group", lambda s: _groups(s["n"]),
     [dict(n=_ragged(g)) for g in BATCH_UNITS], fixed=dict(satd_variant=0, gpw=0), loop="satd_groups_per_wave",
     zero=lambda setting, shape: satd_default_groups(setting.get("satd_variant", 0), shape["n"]), wg="satd_wg_threads")
_row("xSatd8x8BatchDev-dma", "xSatd8x8BatchDev", SATD[1:], "32-block SATD group", lambda s: _groups(s["n"]),
     [dict(n=_ragged(g)) for g in BATCH_UNITS], fixed=dict(satd_variant=0, gpw=0), loop="satd_groups_per_wave",
     zero=lambda setting, shape: 4, wg="satd_wg_threads", base=dict(satd_variant=3))

# the transform set: a wave takes 32x32 tiles of (32 / N)^2 blocks.  The forward's run is fixed at one tile; contiguous 32x32 batches
# are the DCT32 batch kernels' (launch_op), the forward's with "dct32_blocks_per_wave" and "dct32_variant"
SET_CLASSES = ((0, 4), (1, 8), (3, 16), (0, 32))


def _per_tile(shape):
    return (32 // shape["cls"][1]) ** 2


def _set_units(shape):
    return (shape["n"] + _per_tile(shape) - 1) // _per_tile(shape)


def _set_shapes(contiguous32):
    out = []
    for i, u in enumerate(BATCH_UNITS):
        cls = SET_CLASSES[i % 4]
        per = (32 // cls[1]) ** 2
        out.append(dict(cls=cls, n=u * per - (per // 2 if i % 3 == 1 else 0), offsets=cls[1] == 32 or i % 2 == 1))   # a last tile half full
    return out + [dict(cls=(0, 32), n=u, offsets=False) for u in contiguous32]


_row("xTransformFwdBatchDev", "xTransformFwdBatchDev", ("dct32_variant", DCT, "dct32_blocks_per_wave", ADAPTIVE), "32x32 tile of blocks", _set_units,
     _set_shapes(BATCH_UNITS), fixed=dict(wg=0), loop="dct32_blocks_per_wave", live=lambda s: s["cls"][1] == 32 and not s["offsets"], wg=DCT)
_row("xTransformInvBatchDev", "xTransformInvBatchDev", (DCT, "dct32_inv_blocks_per_wave", ADAPTIVE), "32x32 tile of blocks", _set_units,
     _set_shapes((1, 7, 10)) + [dict(cls=(2, 8), n=16 * u - 3, offsets=False) for u in (5, 8, 17, 19, 108)],
     fixed=dict(wg=0), loop="dct32_inv_blocks_per_wave", wg=DCT)
for _inverse in (0, 1):                                                     # 0 = 2: the wave's table copy serves two tiles
    _row("xTransformTilesDev-%s" % ("inv" if _inverse else "fwd"), "xTransformTilesDev", (DCT, "tile_tiles_per_wave", ADAPTIVE), "32x32 tile", _n,
         [dict(inverse=_inverse, n=n, offsets=n % 2 == 0) for n in BATCH_UNITS], fixed=dict(tpw=0), loop="tile_tiles_per_wave",
         zero=lambda setting, shape: 2, wg=DCT)


# ---- tiled frames --------------------------------------------------------------------------------------------------------------------
def _grid(edge, ceil=False):
    def grid(shape):
        w, h = shape["size"]
        return ((h + edge - 1) // edge, (w + edge - 1) // edge) if ceil else (h // edge, w // edge)
    return grid


def _count(edge, per=1, ceil=False):
    grid = _grid(edge, ceil)
    return lambda shape: per * grid(shape)[0] * grid(shape)[1]


def _sizes(*sizes, **more):
    return [dict(size=s, **more) for s in sizes]


# 32x32 blocks in raster order: 1, 7, 5, 6 (two rows of three), 24, and for the loop 2, 8, 10, 18 = 9 * 2 blocks
FRAMES32 = ((32, 32), (224, 32), (160, 32), (96, 64), (192, 128))
FRAMES32_LOOP = FRAMES32 + ((64, 32), (128, 64), (320, 32), (192, 96), (96, 96), (128, 96))
# whole 64x64 CTUs: 1, 2, 3, 6 in two rows, 12; and for one wave per CTU 1, 3, 4, 5, 15 and 24 (the one frame here beyond 320 x 192)
FRAMES64_FIVES = ((64, 64), (128, 64), (192, 64), (192, 128), (256, 192))
FRAMES64 = ((64, 64), (192, 64), (128, 128), (320, 64), (320, 192), (384, 256))
# CTUs of any frame of whole tiles, cut in both directions: 1, 2, 12 (80 x 48 and 208 x 144), 3, 4, 5, 15, 24
FRAMES_CUT = ((16, 16), (80, 48), (208, 144), (144, 48), (80, 80), (304, 48), (304, 144), (368, 208))

_row("xDct32FwdFromTilesDev", "xDct32FwdFromTilesDev", (DCT,), "32x32 luma block", _count(32), _sizes(*FRAMES32), fixed=dict(wg=0), wg=DCT, frame=_grid(32))
_row("xDct32FwdChromaFromTilesDev", "xDct32FwdChromaFromTilesDev", (DCT,), "CTU (both chroma planes)", _count(64),
     [dict(size=s, pitch=1 + i % 2) for i, s in enumerate(FRAMES64)], fixed=dict(wg=0), wg=DCT, frame=_grid(64))
_row("xDct32FwdCtuFromTilesDev", "xDct32FwdCtuFromTilesDev", (DCT,), "a fifth of a CTU", _count(64, 5), _sizes(*FRAMES64_FIVES), fixed=dict(wg=0), wg=DCT,
     frame=_grid(64), fives=True)
_row("xSatd8x8FromTilesDev", "xSatd8x8FromTilesDev", ("satd_variant",), "eight tiles", lambda s: (_count(16)(s) + 7) // 8,
     _sizes((16, 16), (48, 32), (80, 48), (272, 64)), fixed=dict(satd_variant=0), frame=_grid(16))
_row("xDct32InvToTilesDev", "xDct32InvToTilesDev", (DCT, "dct32_inv_blocks_per_wave", ADAPTIVE), "32x32 luma block", _count(32), _sizes(*FRAMES32_LOOP),
     fixed=dict(opt=(2, 0)), loop="dct32_inv_blocks_per_wave", wg=DCT, frame=_grid(32))
_row("xDct32InvCtuToTilesDev", "xDct32InvCtuToTilesDev", (DCT,), "a fifth of a CTU", _count(64, 5), _sizes(*FRAMES64_FIVES), fixed=dict(wg=0), wg=DCT,
     frame=_grid(64), fives=True)
_row("xDct32CodeCtuTilesGpu", "xDct32CodeCtuTilesGpu", (DCT,), "a fifth of a CTU", _count(64, 5), _sizes(*FRAMES64_FIVES), wg=DCT, frame=_grid(64), fives=True)
_row("xTransformCtuFromTilesDev", "xTransformCtuFromTilesDev", (DCT,), "CTU, cut ones included", _count(64, ceil=True), _sizes(*FRAMES_CUT), fixed=dict(wg=0),
     wg=DCT, frame=_grid(64, ceil=True))
_row("xTransformCtuToTilesDev", "xTransformCtuToTilesDev", (DCT,), "CTU, cut ones included", _count(64, ceil=True), _sizes(*FRAMES_CUT), fixed=dict(wg=0),
     wg=DCT, frame=_grid(64, ceil=True))

# ---- the motion searches: "me_tile_rows" is the block rows of a search tile; the SATD searches snap it to 2, 4 or 8, the SAD ones run 2 ----
def _search_tiles(shape):
    w, h = shape["size"]
    return ((w // 8 + 7) // 8) * ((h // 8 + 1) // 2)


PLANAR = [dict(size=(16, 16), costs=True, gap=0), dict(size=(40, 24), costs=False, gap=1), dict(size=(40, 72), costs=True, gap=1)]   # nine block rows: partial tiles at 2, 4 and 8
TILED = [dict(size=(16, 16), costs=True), dict(size=(48, 32), costs=False), dict(size=(48, 80), costs=True)]
for _name, _shapes in (("xSatd8x8SearchDev", PLANAR), ("xSad8x8SearchDev", PLANAR), ("xSatd8x8SearchFromTilesDev", TILED), ("xSad8x8SearchFromTilesDev", TILED)):
    _row(_name, _name, ("me_tile_rows",), "search tile of two block rows", _search_tiles, _shapes, fixed=dict(rows=0))

# ---- a configuration taken, the CU count used: every option of the configuration once -----------------------------------------------
_row("xFillResidualDev", "xFillResidualDev", (), "workgroup of 2048 samples", lambda s: max((s["n"] // 8 + 255) // 256, 1),
     [dict(n=n) for n in (1, 7, 9, 1023, 4109)], fixed=dict(wg=0), pairs=False, unused=(DCT, "dct32_blocks_per_wave", ADAPTIVE))

# ---- the host-pointer calls: launch_op on staged chunks (one chunk at these sizes); up to 64 KiB each way the kernel runs on pinned host memory ----
HOST_DCT = (1, 3, 7, 10, 17, 32, 33, 36, 37)                                          # 33 blocks: the first size on the staged path
_row("xDct32FwdBatch", "xDct32FwdBatch", ROWS["xDct32FwdBatchDev"].options, "32x32 block", _n, [dict(n=n) for n in HOST_DCT],
     loop="dct32_blocks_per_wave", wg=DCT, builder="host")
_row("xDct32InvBatch", "xDct32InvBatch", ROWS["xDct32InvBatchDev"].options, "32x32 block", _n, [dict(n=n) for n in HOST_DCT],
     loop="dct32_inv_blocks_per_wave", wg=DCT, builder="host")
_row("xSatd8x8Batch", "xSatd8x8Batch", SATD, "32-block SATD group", lambda s: _groups(s["n"]), [dict(n=n) for n in (1, 31, 95, 200, 289, 512, 513, 1150, 1153)],
     loop="satd_groups_per_wave", zero=lambda setting, shape: satd_default_groups(setting.get("satd_variant", 0), shape["n"]),
     wg="satd_wg_threads", builder="host")


# ---- the settings of a row ------------------------------------------------------------------------------------------------------------
def _loops(row, setting):
    """the setting names a per-wave value of the row other than its default"""
    return any(k in PER_WAVE and v != DEFAULTS[k] for k, v in setting.items())


def swept(row):
    """the options a row's settings vary: the ones that reach its launch and the ones its configuration merely carries"""
    return tuple(o for o in row.options + row.unused if o not in row.base)


def settings(row):
    """Every option of the row at each of its values, the others at their defaults; "adaptive_per_wave" 0 beside every per-wave value that
    is not the default; every (workgroup size, per-wave value) pair with "adaptive_per_wave" 0; every option at its largest value; and the
    clamp's own path, "adaptive_per_wave" 1 with a per-wave value of 9.  All on top of the row's base."""
    options = swept(row)
    adaptive = ADAPTIVE in options
    out = []

    def add(**opts):
        s = dict(row.base, **opts)
        if adaptive and ADAPTIVE not in opts and _loops(row, s):
            s[ADAPTIVE] = 0
        if s not in out:
            out.append(s)

    add()
    for o in options:
        for v in VALUES[o]:
            add(**{o: v})
    per_wave = [o for o in options if o in PER_WAVE]
    if row.pairs and row.wg:
        for o in per_wave:
            for wg in VALUES[row.wg]:
                for v in VALUES[o]:
                    add(**{row.wg: wg, o: v, ADAPTIVE: 0})
    add(**{o: max(VALUES[o]) for o in options})
    if adaptive and per_wave:
        add(**dict({o: max(VALUES[o]) for o in options}, **{ADAPTIVE: 0}))
        for o in per_wave:
            add(**{o: 9, ADAPTIVE: 1})
    return out


def loop_length(row, setting, shape, cu_count=CU_COUNT):
    """the units one wave of this launch takes (1 for a row or a shape without a loop)"""
    if row.loop is None or not row.live(shape):
        return 1
    value = setting.get(row.loop, DEFAULTS[row.loop]) or row.zero(setting, shape)
    return per_wave_in_force(value, row.units(shape), setting.get(ADAPTIVE, DEFAULTS[ADAPTIVE]), cu_count)


def intended_length(row, setting, shape):
    """what the setting is meant to run: its per-wave value as it stands under "adaptive_per_wave" 0, and one unit per wave under 1 (the
    clamp: none of these shapes has cu_count * 40 * 2 units)"""
    if row.loop is None or not row.live(shape):
        return 1
    if setting.get(ADAPTIVE, DEFAULTS[ADAPTIVE]):
        return 1
    return setting.get(row.loop, DEFAULTS[row.loop]) or row.zero(setting, shape)


# ---- what the shapes of a row have to cover --------------------------------------------------------------------------------------------
def waves_per_wg(row):
    """the workgroup sizes a row runs, in waves"""
    return (1, 2, 3, 4) if row.wg else (row.wg_fixed,)


def one_live_wave_in_the_last_workgroup(counts, w):
    """... behind at least one full workgroup"""
    return any(c % w == 1 and c > w for c in counts)


def one_idle_wave_in_the_last_workgroup(counts, w):
    return any(c % w == w - 1 and c > w for c in counts)


def full_workgroups(counts):
    return any(c % 12 == 0 and c >= 24 for c in counts)


def short_last_run(units, p):
    """the last wave of the launch takes fewer than p units"""
    return units % p != 0


def loop_remainders(units, p):
    """a last run of one unit, a last run one short, a launch smaller than one run, and whole workgroups of whole runs"""
    return {"remainder 1": any(u % p == 1 for u in units), "remainder p - 1": any(u % p == p - 1 for u in units),
            "fewer than p": any(u < p for u in units), "p * W * k": any(u % (p * w) == 0 for u in units for w in (2, 3, 4))}


def straddles(ctus, w):
    """five waves per CTU: some CTU's waves lie in two workgroups of w waves"""
    return any((5 * c) // w != (5 * c + 4) // w for c in range(ctus))


def missing(row):
    """the conditions the row's shapes do not meet, as text (empty: all met).  The waves counted are those of ONE unit per wave -- what
    every launch of these sizes runs while "adaptive_per_wave" is 1, so what the sweep of the workgroup size alone runs -- and the loop
    conditions are those of the per-wave values 2, 3 and 9 on the shapes whose launch has the loop."""
    out = []
    counts = [row.units(s) for s in row.shapes]
    if (5 if row.fives else 1) not in counts:
        out.append("a shape of one unit (five waves per CTU: of one CTU)")
    if not row.wg and row.wg_fixed > 1 and not one_live_wave_in_the_last_workgroup(counts, row.wg_fixed):
        out.append("waves %% %d == 1" % row.wg_fixed)
    if row.wg:
        for w in (2, 3, 4):
            if not one_live_wave_in_the_last_workgroup(counts, w):
                out.append("waves %% %d == 1" % w)
        for w in (3, 4):
            if not one_idle_wave_in_the_last_workgroup(counts, w):
                out.append("waves %% %d == %d" % (w, w - 1))
        if not full_workgroups(counts):
            out.append("waves % 12 == 0, at least 24")
    if row.frame and not any(min(row.frame(s)) >= 2 for s in row.shapes):
        out.append("two rows and two columns of units")
    if row.fives:
        ctus = [row.units(s) // 5 for s in row.shapes]
        for w in (2, 3, 4):
            if not any(straddles(c, w) for c in ctus):
                out.append("a CTU across workgroups of %d waves" % w)
        if not any(row.frame(s)[0] >= 2 for s in row.shapes):
            out.append("two CTU rows")
    if row.loop and row.pairs:
        live = [row.units(s) for s in row.shapes if row.live(s)]
        for p in LOOP_LENGTHS:
            out += ["per-wave %d: %s" % (p, k) for k, met in loop_remainders(live, p).items() if not met]
    return out
