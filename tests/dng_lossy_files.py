"""TEST INFRASTRUCTURE: the lossy-DNG chain (include/rsx.h section 4f) as the composition of the
models its stages are pinned by, and a small case table.

  compose()        dng_post_files.apply (list 1 + look-up) -> scale_files.apply ->
                   dng_post_files.apply (list 2, no table) -> bad_pixels_files.model_fix, with the
                   chain's own rules in between: an OpcodeList2 entry of 0 bytes fails the file, the
                   scale crop is list 1's, the positions merge as mBadPixelPositions does
  decoded()        the image the tiles of a shape decode to, by dng_jpeg_files.model_decode
  cases()          the table both the validation tests and the GPU tests walk

The reference build of this project has no libjpeg, so there is no recording of the chain itself:
each model is held against the reference (or, for JPEG, Pillow's recordings) by its own tests.
"""
import functools

import numpy as np

import bad_pixels_files as B
import dng_jpeg_files as J
import dng_post_files as P
import scale_files as S

OK, INVALID_ARG, IO, UNSUPPORTED, TILE_ERRORS = 0, 1, 2, 7, 9
STAGE1, SCALED, LIST2, FIXED = 1, 2, 4, 8


# ---------------------------------------------------------------------------------------
# the shapes
# ---------------------------------------------------------------------------------------
class Shape:
    def __init__(self, name, dim_x, dim_y, cpp, tiles):
        """tiles: [(fixture name, off_x, off_y)]"""
        self.name, self.dim_x, self.dim_y, self.cpp, self.tiles = name, dim_x, dim_y, cpp, tiles
        self.cfa = cpp == 1

    def streams(self):
        return [J.case(n)["stream"] for n, _, _ in self.tiles]

    def offsets(self):
        return [(x, y) for _, x, y in self.tiles]


def _grid(name, tw, th):
    return [(name, tw * (k % 2), th * (k // 2)) for k in range(4)]


SHAPES = {s.name: s for s in (
    Shape("96x144x3", 96, 144, 3, _grid("444_48x72", 48, 72)),  # tiles exactly: one rectangle
    Shape("80x100x3", 80, 100, 3, _grid("444_48x72", 48, 72)),  # the tiles cut by the image's edge
    Shape("66x100x1", 66, 100, 1, _grid("grey_33x50", 33, 50)),  # CFA, an odd tile width
    Shape("64x96x3", 64, 96, 3, [("restart3_420_64x96", 0, 0)]),  # several entropy segments
)}


@functools.lru_cache(maxsize=None)
def _frame(name):
    c = J.case(name)
    st, got = J.model_decode(c["stream"], c["cpp"])
    assert st == J.OK and J.sha(got) == c["sha256"], name
    return got


@functools.lru_cache(maxsize=None)
def decoded(shape_name):
    """(dim_y, dim_x * cpp) uint16: what the tiles of the shape decode to"""
    s = SHAPES[shape_name]
    img = np.zeros((s.dim_y, s.dim_x * s.cpp), np.uint16)
    for n, x, y in s.tiles:
        J.paste(img, _frame(n), x, y, s.cpp)
    img.setflags(write=False)
    return img


# ---------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, shape, list1=None, table=None, crop=None, list2=None, black=-1,
                 white=None, sep=None, areas=(), dither=True, sse2=True, scale_crop=None, fix=False,
                 bad_cap=1 << 16):
        """list1 / list2: the entries' bytes (list2 None: no OPCODELIST2; b"": an entry of 0 bytes);
        crop: (x, y, w, h) in front of list 1 (None: the image); scale_crop: what the caller puts
        into the scale descriptor (None: list 1's crop, as it must)"""
        self.name, self.shape = name, SHAPES[shape]
        self.list1, self.table, self.list2 = list1, table, list2
        s = self.shape
        self.crop = (0, 0, s.dim_x, s.dim_y) if crop is None else crop
        self.black, self.white, self.sep, self.areas = black, white, sep, list(areas)
        self.dither, self.sse2, self.scale_crop = dither, sse2, scale_crop
        self.fix, self.bad_cap = fix, bad_cap


def _fixed_count(info, data, cpp, crop, full):
    """FixBadPixelsList positions of the applied part of a list"""
    if not data or info["n_applied"] == 0:
        return 0
    ops = P.parse(data, cpp, crop, full)
    return sum(len(op["positions"]) for op in ops[:info["n_applied"]] if op["code"] == 5)


def merge(bad1, bad2, n_fixed2):
    """mBadPixelPositions behind both lists (common/DngOpcodes.cpp:180, :320)"""
    return list(bad2[:n_fixed2]) + list(bad1) + list(bad2[n_fixed2:])


def compose(c, img):
    """The chain on `img` (what the tiles decoded to).  Returns a dict: status, img, stages, info1,
    info2 (None without list 2 or when it did not run), scale (scale_files' result or None), bad
    (merged, or None when they do not fit bad_cap), n_bad1, n_bad2, fixed (n_bad, n_fixed, map or
    None).  A status that ends the call before anything is decoded leaves img None."""
    s = c.shape
    full = (s.dim_x, s.dim_y)
    out = dict(status=OK, img=None, stages=0, info1=None, info2=None, scale=None, bad=None,
               n_bad1=0, n_bad2=0, fixed=(0, 0, None))
    st, img1, info1 = P.apply(img, s.cpp, c.crop, c.list1, c.table)
    out["info1"] = info1
    if st != OK:
        out["status"] = st
        return out
    f1 = _fixed_count(info1, c.list1, s.cpp, c.crop, full)
    f2 = 0
    crop1 = info1["crop"]
    if c.list2 is not None:
        if len(c.list2) == 0:
            out["status"] = IO  # (no `count > 0` guard: getU32 throws)
            return out
        # the verdict needs no pixel
        st2, _, info2 = P.apply(np.zeros_like(img), s.cpp, crop1, c.list2, None)
        if st2 != OK:
            out["status"] = st2
            return out
        out["info2"] = dict(info2, bad=[])
        f2 = _fixed_count(info2, c.list2, s.cpp, crop1, full)
        scale_crop = crop1 if c.scale_crop is None else c.scale_crop
        if tuple(scale_crop) != tuple(crop1):
            out["status"] = INVALID_ARG
            return out
    if c.fix and s.cpp > 1 and (f1 or f2):
        out["status"] = UNSUPPORTED
        return out
    cur, stages, bad2 = img1, STAGE1, []
    refused = False
    if c.list2 is not None:
        sc = S.Case(c.name, img1, s.cpp, s.cfa, crop1, c.black, c.white, c.sep, c.areas, c.dither,
                    c.sse2)
        st, scaled, res = S.apply(sc)
        if st == INVALID_ARG:
            out["status"] = st
            return out
        if st == UNSUPPORTED:  # (from the image's contents: the shapes here are small)
            refused = True
        else:
            out["scale"] = res
            stages |= SCALED
            st2, cur, info2 = P.apply(scaled, s.cpp, crop1, c.list2, None)
            assert st2 == OK
            out["info2"] = info2
            bad2 = info2["bad"]
            stages |= LIST2
    out["n_bad1"], out["n_bad2"] = len(info1["bad"]), len(bad2)
    merged = merge(info1["bad"], bad2, f2)
    fits = len(merged) <= c.bad_cap
    if fits:
        out["bad"] = merged
    if c.fix and fits and not refused:
        assert s.cpp == 1 or not merged
        if merged:
            cur, m, n_bad, n_fixed = B.model_fix(cur, s.cfa, merged)
            out["fixed"] = (n_bad, n_fixed, m)
        stages |= FIXED
    out.update(img=cur, stages=stages, status=UNSUPPORTED if refused or not fits else OK)
    return out


def validate(c):
    """what needs no pixel: (status, info1 or None, info2 or None, the FixBadPixelsList positions
    of both lists in the final order, or None)"""
    s = c.shape
    full = (s.dim_x, s.dim_y)
    zeros = np.zeros((s.dim_y, s.dim_x * s.cpp), np.uint16)
    st, _, info1 = P.apply(zeros, s.cpp, c.crop, c.list1, None)
    if st != OK:
        return st, None, None, None
    f1 = _fixed_count(info1, c.list1, s.cpp, c.crop, full)
    # (zeros: a FixBadPixelsConstant 0 would hit; the table's cases use other constants)
    fixed1 = info1["bad"][:f1]
    info2, fixed2 = None, []
    if c.list2 is not None:
        if len(c.list2) == 0:
            return IO, info1, None, None
        st, _, info2 = P.apply(zeros, s.cpp, info1["crop"], c.list2, None)
        if st != OK:
            return st, info1, None, None
        fixed2 = info2["bad"][:_fixed_count(info2, c.list2, s.cpp, info1["crop"], full)]
        scale_crop = info1["crop"] if c.scale_crop is None else c.scale_crop
        if tuple(scale_crop) != tuple(info1["crop"]):
            return INVALID_ARG, info1, info2, None
        sc = S.Case(c.name, zeros, s.cpp, s.cfa, info1["crop"], c.black, c.white, c.sep, c.areas,
                    c.dither, c.sse2)
        if c.sep is None and info1["crop"][2] and info1["crop"][3]:
            for off, size, vert in sc.areas:
                if off + (size - (size & 1)) > (sc.w if vert else sc.h):
                    return INVALID_ARG, info1, info2, None
    if c.fix and s.cpp > 1 and (fixed1 or fixed2):
        return UNSUPPORTED, info1, info2, None
    if len(fixed1) + len(fixed2) > c.bad_cap:
        return UNSUPPORTED, info1, info2, None
    return OK, info1, info2, fixed2 + fixed1


def _tables():
    rng = np.random.default_rng(0x884C)
    t14 = np.sort(rng.integers(300, 16384, size=256)).astype(np.uint16)  # 8 bits -> 14 bits
    t10 = np.sort(rng.integers(20, 1000, size=256)).astype(np.uint16)  # white - black < 1041
    t64k = rng.integers(0, 65536, size=65536).astype(np.uint16)
    return rng, t14, t10, t64k


@functools.lru_cache(maxsize=None)
def cases():
    rng, t14, t10, t64k = _tables()
    L = P.opcode_list
    d = lambda n, lo, hi: rng.uniform(lo, hi, size=n).astype(np.float32)  # noqa: E731
    lev = dict(black=256, white=16383)
    pts1, pts2 = [(3, 5), (50, 33), (99, 65)], [(0, 0), (49, 32)]
    return [
        # no list 2: the _post / _finish equivalent
        Case("post_rgb", "96x144x3", L([P.op_table((1, 3, 140, 90), t64k, planes=(1, 2), pitch=(2, 3))]),
             t14),
        Case("post_rgb_cut", "80x100x3", None, t14),
        Case("finish_cfa", "66x100x1", L([P.op_bad_list(pts1, [(10, 20, 12, 23)]), P.op_bad_constant(196)]),
             t14, fix=True),
        Case("finish_segments_no_positions", "64x96x3", None, t14, fix=True),
        # list 2, the SSE2 variant
        Case("maptable_sse2_dither", "96x144x3", None, t14,
             list2=L([P.op_table((0, 0, 144, 96), t64k, planes=(0, 3))]), **lev),
        Case("deltarow_sse2_plain_rows", "80x100x3", None, t14,
             list2=L([P.op_delta(10, (1, 2, 99, 79), d(98, -0.2, 0.2), planes=(0, 2))]), dither=False, **lev),
        Case("cfa_sse2_row_tail", "66x100x1", None, t14,
             list2=L([P.op_table((0, 0, 100, 66), t64k, pitch=(1, 2))]), **lev),
        # TrimBounds in list 1 moves the scale crop; ScalePerColumn in list 2; the plain variant
        Case("trim_scalecol_plain_dither", "96x144x3",
             L([P.op_trim((2, 5, 141, 92)), P.op_table((0, 0, 139, 87), t64k, planes=(2, 1))]), t14,
             list2=L([P.op_delta(13, (0, 0, 139, 87), d(87, 0.5, 1.5), planes=(0, 3))]), sse2=False, **lev),
        Case("trim_scalecol_plain_cfa", "66x100x1", L([P.op_trim((1, 3, 98, 64))]), t14,
             list2=L([P.op_delta(13, (0, 1, 97, 61), d(30, 0.5, 1.5), pitch=(1, 2))]), sse2=False,
             dither=False, **lev),
        # app_scale >= 63 takes the plain variant although the host has SSE2
        Case("app_scale_plain", "64x96x3", None, t10,
             list2=L([P.op_table((0, 0, 96, 64), t64k, planes=(0, 3))]), black=10, white=1000,
             dither=False),
        Case("app_scale_plain_dither", "66x100x1", None, t10,
             list2=L([P.op_delta(10, (0, 0, 100, 66), d(100, -0.1, 0.1))]), black=10, white=1000),
        Case("separate_levels", "66x100x1", None, t14, list2=L([P.op_table((0, 0, 100, 66), t64k)]),
             white=16000, sep=(260, 270, 280, 290)),
        Case("separate_levels_rgb", "80x100x3", None, t14,
             list2=L([P.op_delta(12, (0, 0, 100, 80), d(100, 0.5, 1.2), planes=(1, 1))]),
             white=16000, sep=(260, 270, 280, 290), dither=False),
        Case("black_area", "66x100x1", None, t14, list2=L([P.op_table((0, 0, 100, 66), t64k)]),
             black=0, white=65535, areas=[(0, 4, False), (2, 6, True)]),
        # the skip rule: list 2 on the unscaled image
        Case("skip_rule", "96x144x3", None, t14,
             list2=L([P.op_table((0, 0, 144, 96), t64k, planes=(0, 3))]), black=0, white=65535),
        # positions: a constant of list 2 that exists only behind the scaling (saturated pixels),
        # both lists with a FixBadPixelsList
        Case("const2_fix", "66x100x1", L([P.op_bad_list(pts1), P.op_bad_constant(53)]), t14,
             list2=L([P.op_bad_constant(65535), P.op_bad_list(pts2, [(70, 60, 72, 66)])]), black=256,
             white=14600, fix=True),
        Case("const2_no_fix", "66x100x1", L([P.op_bad_list(pts1), P.op_bad_constant(53)]), t14,
             list2=L([P.op_bad_constant(65535), P.op_bad_list(pts2)]), black=256, white=14600),
        Case("const2_cap_too_small", "66x100x1", L([P.op_bad_list(pts1), P.op_bad_constant(53)]), t14,
             list2=L([P.op_bad_constant(65535), P.op_bad_list(pts2)]), black=256, white=14600,
             fix=True, bad_cap=6),
        # a list 2 that is logged and a list 2 that stops at a setup()
        Case("list2_fails_constructed", "80x100x3", None, t14,
             list2=L([P.op_table((0, 0, 100, 80), t64k), P.op_table((0, 0, 101, 80), t64k)]), **lev),
        Case("list2_stops_at_setup", "80x100x3", None, t14,
             list2=L([P.op_table((0, 0, 100, 80), t64k, planes=(0, 3)), P.op_bad_constant(7),
                      P.op_table((0, 0, 100, 80), t64k)]), **lev),
        # the scale stage refuses from the image: white below the black level of an area
        Case("scale_refuses", "66x100x1", L([P.op_bad_constant(53)]), t14,
             list2=L([P.op_table((0, 0, 100, 66), t64k)]), black=0, white=200,
             areas=[(0, 4, False)], fix=True),
        # ... with a FixBadPixelsList in the list 2 that never runs: none of its positions comes back
        Case("scale_refuses_list2_positions", "66x100x1", L([P.op_bad_list(pts1), P.op_bad_constant(53)]),
             t14, list2=L([P.op_bad_list(pts2, [(70, 60, 72, 66)]), P.op_table((0, 0, 100, 66), t64k)]),
             black=0, white=200, areas=[(0, 4, False)], fix=True),
        Case("scale_refuses_list2_positions_no_fix", "66x100x1",
             L([P.op_bad_list(pts1), P.op_bad_constant(53)]), t14,
             list2=L([P.op_bad_list(pts2, [(70, 60, 72, 66)]), P.op_table((0, 0, 100, 66), t64k)]),
             black=0, white=200, areas=[(0, 4, False)]),
    ]


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """compose() of a case on its shape's decoded image, computed once and shared"""
    c = case(name)
    out = compose(c, decoded(c.shape.name))
    if out["img"] is not None:
        out["img"].setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------
# descriptors (rawspeed_amd.abi)
# ---------------------------------------------------------------------------------------
def desc(c, abi):
    """(abi.DngLossyDesc, keep-alive) of a case"""
    stage1 = abi.dng_post_desc(c.list1, c.table, c.crop)
    scale = None
    if c.list2 is not None:
        scale = scale_desc(c, abi, c.scale_crop)
    return abi.dng_lossy_desc(stage1, c.list2, scale, c.fix)


def scale_desc(c, abi, crop):
    if crop is None:
        st, info1, _, _ = validate(Case(c.name, c.shape.name, c.list1, c.table, c.crop))
        crop = info1["crop"] if info1 else c.crop
    return abi.scale_desc(crop, c.black, c.white, c.sep, c.areas, c.dither, c.sse2)
