"""The case table of the gray move kernels (csrc/kernels_move.hip), and a
numpy restatement of what they compute.

test_move_gpu.py runs every case through uphip_move_probe and compares image
and row counts with the oracle (center_mask -> apply_masks -> align_mask).
test_move_cases.py (no GPU) checks the table itself: that the restatement
below equals the oracle on every case, that no case is a no-op, and that the
classes of geometry the kernels' address arithmetic distinguishes are all met.

A case holds the two moves in the reference's terms -- centre: the point and
the area given to center_mask; align: inside, outside, alignment and margin
given to align_mask -- and the raw target of each follows by the arithmetic of
k_center_args / k_border_assemble (center_raw / align_raw).

The restatement (sources) follows the reference's three steps literally --
copy the clipped area out into a background-filled image, wipe the area, copy
that image back at the target -- on a plane of symbols instead of bytes: every
output pixel ends as R[y', x'] (a pixel of the page), the centring's
background, the align move's background or the mask colour.  It is used for
coverage facts only (facts), never for expected pixels.

The folded mask's contract: k_move_rect_g16 with a mask and k_move_chain_g16
mask the pixels the align move keeps, not the ones it moves, which is
apply_masks + align_mask where the moved area lies inside the mask.  A batch
gives the detected border as both; the table keeps clip(inside) inside the
mask wherever the align move is active (Case checks it).
"""
import types

import numpy as np

from unpaper_hip import ctypes_abi as A
from unpaper_hip.hostimage import HostImage

PLAIN, COUNT, DRY, MASKED, TWO_PASS, CHAIN = (A.MOVE_PLAIN, A.MOVE_COUNT, A.MOVE_DRY,
                                              A.MOVE_MASKED, A.MOVE_TWO_PASS, A.MOVE_CHAIN)
ROUTE_NAMES = {PLAIN: "plain", COUNT: "count", DRY: "dry", MASKED: "masked",
               TWO_PASS: "two_pass", CHAIN: "chain"}
COUNTING = (COUNT, DRY, TWO_PASS, CHAIN)
FAMILIES = ("realignment", "breakpoints", "rows", "degenerate", "chain", "counts")
THRESHOLDS = (0, 127, 170, 254, 255)
# width x height: the smallest at which each structure of the kernels exists
SIZES = {
    (7, 5): "one partial vector only, fewer rows than a wave's eight",
    (16, 8): "no partial vector, one wave's rows",
    (48, 33): "crosses the 32-row block and 8-row wave bounds",
    (97, 61): "general",
    (97, 100): "row ranges [0,40) + [61,100) of a dry pass",
    (1043, 40): "second lane pass of k_move_chain_g16 (1024 columns a pass)",
    (3089, 34): "second chunk of k_move_rect_g16 (3072 columns a chunk)",
}
BLOCK_ROWS = 32      # kMoveBlockRows, kChainRows
KIND_R, KIND_BG1, KIND_BG2, KIND_MASK = 0, 1, 2, 3
_GRAYS = (37, 91, 143, 201, 254, 1, 128, 171)   # none is 0: the row padding is


# ------------------------------------------------------------ rectangles
def normalize(r):
    x0, y0, x1, y1 = r
    return (min(x0, x1), min(y0, y1), max(x0, x1), max(y0, y1))


def clip(r, W, H):
    n = normalize(r)
    return (max(n[0], 0), max(n[1], 0), min(n[2], W - 1), min(n[3], H - 1))


def cdiv2(a):
    """C's a / 2 (towards zero)."""
    return -((-a) // 2) if a < 0 else a // 2


class Raw(types.SimpleNamespace):
    """A move as the kernels take it (MoveArgs)."""


def _identity(area, tx, ty, W, H):
    n = normalize(area)
    return (n[0], n[1]) == (area[0], area[1]) and clip(area, W, H) == n and (tx, ty) == (n[0], n[1])


def center_raw(W, H, c, bg):
    """k_center_args: the target centres the area's size on the point; the
    move applies only where the whole target lies inside the image."""
    if c is None:
        return Raw(area=(0, 0, 0, 0), tx=0, ty=0, bg=bg, active=0)
    x0, y0, x1, y1 = c["area"]
    sw, sh = abs(x0 - x1) + 1, abs(y0 - y1) + 1
    tx, ty = c["point"][0] - sw // 2, c["point"][1] - sh // 2
    inside = tx >= 0 and ty >= 0 and tx + sw <= W and ty + sh <= H
    active = inside and (c.get("force", False) or not _identity(c["area"], tx, ty, W, H))
    return Raw(area=tuple(c["area"]), tx=tx, ty=ty, bg=bg, active=int(active))


def align_raw(W, H, a, bg):
    """k_border_assemble: align_mask's target (masks.c:265-290)."""
    if a is None:
        return Raw(area=(0, 0, 0, 0), tx=0, ty=0, bg=bg, active=0)
    m, o = a["inside"], a["outside"]
    iw, ih = abs(m[0] - m[2]) + 1, abs(m[1] - m[3]) + 1
    left, top, right, bottom = a["alignment"]
    mh, mv = a["margin"]
    if left:
        tx = o[0] + mh
    elif right:
        tx = o[2] - iw - mh
    else:
        tx = cdiv2(o[0] + o[2] - iw)
    if top:
        ty = o[1] + mv
    elif bottom:
        ty = o[3] - ih - mv
    else:
        ty = cdiv2(o[1] + o[3] - ih)
    active = a.get("force", False) or not _identity(m, tx, ty, W, H)
    return Raw(area=tuple(m), tx=tx, ty=ty, bg=bg, active=int(active))


def center_to(area, tx, ty, force=False):
    """The centre point that sends `area` to (tx, ty)."""
    sw, sh = abs(area[0] - area[2]) + 1, abs(area[1] - area[3]) + 1
    return {"area": tuple(area), "point": (tx + sw // 2, ty + sh // 2), "force": force}


def align_to(area, tx, ty, mode="lt", force=False):
    """inside / outside / alignment / margin that send `area` to (tx, ty):
    left+top with the margin carrying the target, right+bottom against an
    outside rectangle, or centred in one."""
    iw, ih = abs(area[0] - area[2]) + 1, abs(area[1] - area[3]) + 1
    if mode == "lt":
        a = {"outside": (3, 2, 90, 50), "alignment": (1, 1, 0, 0), "margin": (tx - 3, ty - 2)}
    elif mode == "rb":
        a = {"outside": (1, 1, tx + iw + 4, ty + ih + 6), "alignment": (0, 0, 1, 1),
             "margin": (4, 6)}
    else:
        a = {"outside": (tx, ty, tx + iw, ty + ih), "alignment": (0, 0, 0, 0), "margin": (9, 9)}
    a["inside"] = tuple(area)
    a["force"] = force
    return a


# ------------------------------------------------------------------ cases
class Case:
    def __init__(self, family, tag, size, route, center=None, align=None, mask=None, seed=0,
                 rx=None, thr=170, ranges=(0, 0, 0, 0), only=-1, classes=(), identity=None):
        assert family in FAMILIES and tuple(size) in SIZES
        self.family, self.route = family, route
        self.W, self.H = size
        self.id = "%s-%s-%dx%d-%s" % (family, ROUTE_NAMES[route], self.W, self.H, tag)
        self.center, self.align, self.mask = center, align, mask
        self.seed = seed
        self.bg1, self.bg2, self.mcol = (_GRAYS[seed % 8], _GRAYS[(seed + 3) % 8],
                                         _GRAYS[(seed + 5) % 8])
        self.rx = tuple(rx) if rx is not None else (0, self.W - 1)
        self.thr = thr
        self.ranges, self.only = tuple(ranges), only
        self.classes = tuple(classes)
        self.identity = identity      # the reason a case leaves the page as it is
        if route in (PLAIN, COUNT, DRY):
            assert align is None and mask is None
        if route == MASKED:
            assert center is None
        self.m1 = center_raw(self.W, self.H, center, self.bg1)
        self.m2 = align_raw(self.W, self.H, align, self.bg2)
        if self.m2.active and mask is not None:   # the folded mask's contract
            a, k = clip(self.m2.area, self.W, self.H), normalize(mask)
            if a[0] <= a[2] and a[1] <= a[3]:
                assert k[0] <= a[0] and k[1] <= a[1] and k[2] >= a[2] and k[3] >= a[3], self.id
        assert 0 <= self.rx[0] and self.rx[1] < self.W
        for m in (self.m1, self.m2):   # see _S: no area wholly below the image
            assert not m.active or normalize(m.area)[1] <= self.H - 1, self.id

    def __repr__(self):
        return self.id

    @property
    def forced(self):
        """Which moves are identities given as active (a batch would switch
        them off): the probe must give the same with active = 0."""
        return (bool(self.center and self.center["force"] and self.m1.active),
                bool(self.align and self.align["force"] and self.m2.active))

    def page(self):
        """Uniform random bytes, so that any misplaced byte shows; thr and
        thr + 1 planted in the first counted column."""
        rng = np.random.default_rng(self.seed * 7919 + self.W * 31 + self.H)
        arr = rng.integers(0, 256, size=(self.H, self.W), dtype=np.uint8)
        arr[0, self.rx[0]] = self.thr
        if self.thr < 255:
            arr[1, self.rx[0]] = self.thr + 1
        return HostImage.from_array(arr, A.FMT_GRAY8)

    def probe(self, route=None, center_active=None, align_active=None):
        p = A.MoveProbe()
        p.route = self.route if route is None else route
        for step, m in ((p.center, self.m1), (p.align, self.m2)):
            step.area = A.rect(*m.area)
            step.tx, step.ty = m.tx, m.ty
            step.bg = A.pixel(m.bg)
            step.active = m.active
        if center_active is not None:
            p.center.active = center_active
        if align_active is not None:
            p.align.active = align_active
        p.mask_count = 0 if self.mask is None else 1
        if self.mask is not None:
            p.mask = A.rect(*self.mask)
        p.mask_color = A.pixel(self.mcol)
        p.rx0, p.rx1 = self.rx
        p.thr = self.thr
        p.ya0, p.ya1, p.yb0, p.yb1 = self.ranges
        p.only = self.only
        if p.route not in (DRY, CHAIN):
            p.ya0 = p.ya1 = p.yb0 = p.yb1 = 0
            p.only = -1
        return p

    # -- the oracle's planes: the page, the centred plane C, the result -------
    def oracle_planes(self, oracle):
        h = self.page()
        page = h.payload().copy()
        if self.center is not None and self.route != MASKED:
            h.background = (self.bg1,) * 3
            oracle.center_mask(h, A.Point(*self.center["point"]), A.rect(*self.center["area"]))
        centred = h.payload().copy()
        if self.route in (MASKED, TWO_PASS, CHAIN):
            if self.mask is not None:
                oracle.apply_masks(h, [A.rect(*self.mask)], A.pixel(self.mcol))
            if self.align is not None:
                h.background = (self.bg2,) * 3
                p = A.MaskAlignmentParameters()
                p.alignment = A.Edges(*[bool(v) for v in self.align["alignment"]])
                p.margin = A.Delta(*self.align["margin"])
                oracle.align_mask(h, A.rect(*self.align["inside"]),
                                  A.rect(*self.align["outside"]), p)
        return page, centred, h.payload().copy()

    def counted_rows(self, route=None):
        """Mask of the rows a counting route writes."""
        route = self.route if route is None else route
        rows = np.ones(self.H, bool)
        if route in (DRY, CHAIN):
            ya0, ya1, yb0, yb1 = self.ranges
            if ya1 > ya0 or yb1 > yb0:
                rows[:] = False
                rows[ya0:max(ya0, ya1)] = True
                rows[yb0:max(yb0, yb1)] = True
            if self.only == 0:
                rows[:] = False
        return rows

    def expected_rows(self, centred, route=None):
        """(C[y, rx0 : rx1 + 1] <= thr).sum() of the oracle's centred plane;
        the sentinel in the rows a dry pass leaves out."""
        n = (centred[:, self.rx[0]:self.rx[1] + 1] <= self.thr).sum(axis=1).astype(np.uint32)
        return np.where(self.counted_rows(route), n, np.uint32(A.MOVE_ROW_UNWRITTEN))


# ------------------------------------------------------------ restatement
def _fresh(W, H):
    s = np.zeros((4, H, W), np.int32)      # kind, source row, source column, moves passed
    s[1], s[2] = np.indices((H, W))
    return s


def _sym_move(s, area, tx, ty, kind):
    """copy clip(area) out into a `kind`-filled image of the area's size, wipe
    clip(area) with `kind`, copy the image back at (tx, ty) (pixels outside
    the plane dropped)."""
    _, H, W = s.shape
    n = normalize(area)
    sw, sh = n[2] - n[0] + 1, n[3] - n[1] + 1
    a = clip(area, W, H)
    new = np.zeros((4, sh, sw), np.int32)
    new[0] = kind
    new[1:3] = -1
    if a[0] <= a[2] and a[1] <= a[3]:
        out = s[:, a[1]:a[3] + 1, a[0]:a[2] + 1].copy()
        out[3] += 1
        new[:, :a[3] - a[1] + 1, :a[2] - a[0] + 1] = out
        s[0, a[1]:a[3] + 1, a[0]:a[2] + 1] = kind
        s[1:3, a[1]:a[3] + 1, a[0]:a[2] + 1] = -1
    x0, y0, x1, y1 = max(tx, 0), max(ty, 0), min(tx + sw, W), min(ty + sh, H)
    if x1 > x0 and y1 > y0:
        s[:, y0:y1, x0:x1] = new[:, y0 - ty:y1 - ty, x0 - tx:x1 - tx]


def sources(case):
    """(centred, result): per pixel kind / source row / source column / moves
    passed, of the centred plane and of the route's result."""
    W, H = case.W, case.H
    s = _fresh(W, H)
    if case.center is not None and case.route != MASKED:
        m = center_raw(W, H, case.center, 0)
        n = normalize(m.area)
        sw, sh = n[2] - n[0] + 1, n[3] - n[1] + 1
        # center_mask moves only where both corners of the target are inside
        if m.tx >= 0 and m.ty >= 0 and m.tx + sw - 1 <= W - 1 and m.ty + sh - 1 <= H - 1:
            _sym_move(s, m.area, m.tx, m.ty, KIND_BG1)
    centred = s.copy()
    if case.route in (MASKED, TWO_PASS, CHAIN):
        if case.mask is not None:
            k = normalize(case.mask)
            ys, xs = np.indices((H, W))
            out = ~((xs >= k[0]) & (xs <= k[2]) & (ys >= k[1]) & (ys <= k[3]))
            s[0][out] = KIND_MASK
            s[1][out] = s[2][out] = -1
        if case.align is not None:
            m = align_raw(W, H, case.align, 0)
            _sym_move(s, m.area, m.tx, m.ty, KIND_BG2)
    return centred, s


def render(s, page, case):
    consts = np.array([0, case.bg1, case.bg2, case.mcol], np.uint8)
    out = consts[s[0]]
    r = s[0] == KIND_R
    out[r] = page[s[1][r], s[2][r]]
    return out


# ------------------------------------------------------------------- facts
def _geom(W, H, m):
    n, a = normalize(m.area), clip(m.area, W, H)
    return types.SimpleNamespace(n=n, a=a, aw=a[2] - a[0] + 1, ah=a[3] - a[1] + 1,
                                 sw=n[2] - n[0] + 1, sh=n[3] - n[1] + 1, delta=a[0] - m.tx,
                                 tx=m.tx, ty=m.ty)


def _vectors(s):
    """Per (row, whole 16-column vector): (all 16 columns are one constant,
    all 16 are one run of R, the run's column offset, the moves every one of
    its pixels passed or -1)."""
    kind, sy, sx, hops = s
    H, W = kind.shape
    nv = W // 16
    ys, xs = np.indices((H, W))

    def v(a):
        return a[:, :nv * 16].reshape(H, nv, 16)

    def same(a):
        return (a == a[:, :, :1]).all(axis=2)
    k, dx, dy, hp = v(kind), v(sx - xs), v(sy - ys), v(hops)
    const = same(k) & (k[:, :, 0] != KIND_R)
    run = (k == KIND_R).all(axis=2) & same(dx) & same(dy)
    return const, run, dx[:, :, 0], np.where(same(hp), hp[:, :, 0], -1)


def _move_facts(g, W, H, m, mk, F):
    """Facts of one active move under group g (plain, count, masked, chain)."""
    q = _geom(W, H, m)
    bps = {"tx": q.tx, "txsw": q.tx + q.sw, "ax0": q.a[0], "ax1": q.a[2] + 1}
    if q.aw < q.sw:
        bps["txaw"] = q.tx + q.aw
    if mk is not None:
        bps["mk0"], bps["mk1"] = mk[0], mk[2] + 1
    inner = lambda b: 0 < b < W and b % 16 != 0   # noqa: E731
    for name, b in bps.items():
        if b <= 0 or b >= W:
            F.add("%s.bp.%s.off" % (g, name))
            continue
        F.add("%s.bp.%s.%s" % (g, name, "inside" if b % 16 else "on16"))
        if inner(b) and any(inner(o) and o != b and o // 16 == b // 16 for o in bps.values()):
            F.add("%s.bp.%s.multi" % (g, name))
        if W % 16 and b > (W & ~15):
            F.add("%s.bp.%s.tail" % (g, name))
    some = q.aw > 0 and q.ah > 0
    if some:
        for side, off in (("l", q.n[0] < 0), ("r", q.n[2] > W - 1), ("t", q.n[1] < 0),
                          ("b", q.n[3] > H - 1)):
            if off:
                F.add("%s.hang.area.%s" % (g, side))
    seen = q.tx < W and q.tx + q.sw > 0 and q.ty < H and q.ty + q.sh > 0
    if seen:
        for side, off in (("l", q.tx < 0), ("r", q.tx + q.sw > W), ("t", q.ty < 0),
                          ("b", q.ty + q.sh > H)):
            if off:
                F.add("%s.hang.target.%s" % (g, side))
        if q.ty < 0:
            F.add(g + ".rows.ty_neg")
        if q.ty + q.sh > H:
            F.add(g + ".rows.ty_over")
    if some:
        ox = min(q.a[2], q.tx + q.sw - 1) - max(q.a[0], q.tx) + 1
        oy = min(q.a[3], q.ty + q.sh - 1) - max(q.a[1], q.ty) + 1
        if (q.tx, q.ty) == (q.a[0], q.a[1]) and q.a == q.n:
            F.add(g + ".overlap.equal")
        elif ox > 0 and oy > 0:
            if ox <= 4 or oy <= 4:
                F.add(g + ".overlap.partial")      # by a few pixels
        else:
            F.add(g + ".overlap.disjoint")
        if q.a[1] // 8 != q.a[3] // 8:
            F.add(g + ".rows.cross8")
        if q.a[1] // 32 != q.a[3] // 32:
            F.add(g + ".rows.cross32")
    if H < 8:
        F.add(g + ".rows.h_lt8")
    if m.area[0] > m.area[2]:
        F.add(g + ".degen.inv_x")
    if m.area[1] > m.area[3]:
        F.add(g + ".degen.inv_y")
    if q.sw == 1 and q.sh == 1:
        F.add(g + ".degen.one_px")
    for side, off in (("l", q.n[2] < 0), ("r", q.n[0] > W - 1), ("t", q.n[3] < 0),
                      ("b", q.n[1] > H - 1)):
        if off:
            F.add("%s.degen.out_%s" % (g, side))


def _mask_facts(g, W, H, case, F):
    if case.mask is None:
        F.add(g + ".degen.no_mask")
        return
    k = normalize(case.mask)
    if tuple(case.mask) != k:
        F.add(g + ".degen.mask_inv")
    if k[0] <= 0 and k[1] <= 0 and k[2] >= W - 1 and k[3] >= H - 1:
        F.add(g + ".degen.mask_all")


def chain_breakpoints(W, H, m1, m2, mk):
    """The columns k_move_chain_g16 collects: where some stage's class can
    change, sorted, unique, inside (0, W)."""
    b = []
    d2 = 0
    if m2.active:
        q = _geom(W, H, m2)
        b += [q.tx, q.tx + q.aw, q.tx + q.sw, q.a[0], q.a[2] + 1]
        d2 = q.delta
    if mk is not None:
        b += [mk[0], mk[2] + 1]
    if m1.active:
        q = _geom(W, H, m1)
        for v in (q.tx, q.tx + q.aw, q.tx + q.sw, q.a[0], q.a[2] + 1):
            b.append(v)
            if m2.active:
                b.append(v - d2)
    return sorted({v for v in b if 0 < v < W})


def _chain_facts(case, s, F):
    """Facts of the chained gather, per block of 32 rows as the kernel works:
    the breakpoints it keeps (those across which some row's source changes),
    the vectors it writes whole, and the two byte paths."""
    W, H = case.W, case.H
    mk = normalize(case.mask) if case.mask is not None else None
    bps = chain_breakpoints(W, H, case.m1, case.m2, mk)
    assert len(bps) <= 17
    kind, sy, sx, hops = s
    ys, xs = np.indices((H, W))
    dx, dy = sx - xs, sy - ys
    const, run, vdx, vhp = _vectors(s)
    nv = W // 16
    for y0 in range(0, H, BLOCK_ROWS):
        rows = slice(y0, min(y0 + BLOCK_ROWS, H))

        def differs(c0, c1):   # per row of the block: columns c0, c1 have different sources
            return (kind[rows, c0] != kind[rows, c1]) | \
                ((kind[rows, c0] == KIND_R) & ((dx[rows, c0] != dx[rows, c1]) |
                                               (dy[rows, c0] != dy[rows, c1])))
        live = [b for b in bps if differs(b - 1, b).any()]
        starts = [0] + bps                     # interval i of the full list starts here
        whole = []                             # vectors written whole: no kept breakpoint inside
        for vi in range((W + 15) // 16):
            x0 = 16 * vi
            il = sum(1 for b in live if b <= x0)
            ih = sum(1 for b in live if b <= min(x0 + 15, W - 1))
            if x0 + 16 <= W and il == ih:
                whole.append(vi)
                # read through the unmapped index, the vector's cell would be
                # that of interval `il` of the full list
                if il < len(starts) and len(live) < len(bps) and differs(starts[il], x0).any():
                    F.add("chain.live_drop")
                continue
            if ih - il == 3:
                F.add("chain.bytes.three_bp")
            if ih - il >= 4:
                F.add("chain.bytes.many_bp")
        for p0 in range(0, nv, 64):            # a lane pass: 64 vectors, one row a time
            lanes = [vi for vi in whole if p0 <= vi < p0 + 64]
            if not lanes:
                continue
            assert (const[rows][:, lanes] | run[rows][:, lanes]).all(), case.id
            # the lanes holding a run of R pick the realignment path together
            isrun = run[rows][:, lanes]
            r16 = vdx[rows][:, lanes] & 15
            for row_run, row_r in zip(isrun, r16):
                got = set(row_r[row_run].tolist())
                if len(got) == 1:
                    F.add("chain.uniform.%d" % got.pop())
                elif len(got) > 1:
                    F.add("chain.per_lane")
            two = run[rows][:, lanes] & (vhp[rows][:, lanes] == 2)
            for r in np.unique((vdx[rows][:, lanes] & 15)[two]):
                F.add("chain.realign.%d" % r)
            if p0 >= 64 and (run[rows][:, lanes] & (vhp[rows][:, lanes] > 0)).any():
                F.add("chain.pass2")
    if case.m1.active and case.m2.active:
        d1, d2 = _geom(W, H, case.m1).delta, _geom(W, H, case.m2).delta
        if (d1 - d2) % 16 and (run & (vhp == 2)).any():
            F.add("chain.realign.differ")
    if not case.m1.active and case.m2.active:
        F.add("chain.center_inactive")
    if case.m1.active and not case.m2.active:
        F.add("chain.align_inactive")
    if not case.m1.active and not case.m2.active and case.mask is not None:
        F.add("chain.both_inactive_mask")


def facts(case):
    """The classes a case meets, from its arguments and the restatement's
    source map; nothing here comes from a kernel."""
    W, H = case.W, case.H
    F = set()
    centred, s = sources(case)
    g = {PLAIN: "plain", COUNT: "count", DRY: "dry", MASKED: "masked",
         TWO_PASS: "chain", CHAIN: "chain"}[case.route]
    mk = normalize(case.mask) if case.mask is not None else None
    if case.route in (PLAIN, COUNT, DRY):
        moves = [(case.m1, None, centred)]
    elif case.route == MASKED:
        moves = [(case.m2, mk, s)]
        _mask_facts(g, W, H, case, F)
    else:
        moves = [(case.m1, None, centred), (case.m2, mk, s)]
        _mask_facts(g, W, H, case, F)
    for m, k, plane in moves:
        if not m.active:
            continue
        _move_facts(g, W, H, m, k, F)
        if g != "chain":
            # a vector of moved pixels only: two aligned loads realigned by
            # (clip(area).x0 - tx) mod 16
            q = _geom(W, H, m)
            _, run, vdx, vhp = _vectors(plane)
            moved = run & (vhp == 1)
            if moved.any():
                assert (vdx[moved] == q.delta).all()
                F.add("%s.realign.%d.%s" % (g, q.delta & 15, "off" if q.a[0] % 16 else "on"))
                if moved[:, 192:].any():
                    F.add(g + ".chunk2")
    if case.route == MASKED and not case.m2.active and mk is not None:
        # the identity move: the mask applied in place, its columns as bit masks
        w = mk[2] - mk[0] + 1
        if 1 <= w <= 15:
            F.add("inplace.mask.narrow")
        for b in (mk[0], mk[2] + 1):
            if 0 < b < W:
                F.add("inplace.mask." + ("inside" if b % 16 else "on16"))
                if W % 16 and b > (W & ~15):
                    F.add("inplace.mask.tail")
    if case.route == CHAIN:
        _chain_facts(case, s, F)
    if case.route in COUNTING:
        c = "count" if case.route in (COUNT, TWO_PASS) else "dry"
        F.add("%s.thr.%d" % (c, case.thr))
        rx0, rx1 = case.rx
        if (rx0, rx1) == (0, W - 1):
            F.add(c + ".cols.full")
        if rx0 == rx1:
            F.add(c + ".cols.single")
        if rx0 < rx1 and rx0 // 16 == rx1 // 16:
            F.add(c + ".cols.one_vector")
        if rx0 % 16 == 0 and (rx1 + 1) % 16 == 0:
            F.add(c + ".cols.on16")
        if not case.m1.active:
            F.add(c + ".inactive")
        if case.route in (DRY, CHAIN):
            ya0, ya1, yb0, yb1 = case.ranges
            a, b = ya1 > ya0, yb1 > yb0
            if a and b:
                F.add("dry.ranges." + ("unaligned" if any(v % 32 for v in case.ranges)
                                       else "aligned"))
            if a != b:
                F.add("dry.ranges.one_empty")
            F.add("dry.only.%s" % {-1: "none", 0: "0"}.get(case.only, "1"))
    return F


def required():
    """Every class the table must meet."""
    R = []
    for g in ("plain", "count", "masked"):
        R += ["%s.realign.%d.%s" % (g, r, o) for r in range(16) for o in ("on", "off")]
        R.append(g + ".chunk2")
    R += ["chain.realign.%d" % r for r in range(16)]
    R += ["chain.uniform.%d" % r for r in range(16)]
    R += ["chain.realign.differ", "chain.per_lane", "chain.pass2", "chain.live_drop",
          "chain.bytes.three_bp", "chain.bytes.many_bp", "chain.center_inactive",
          "chain.align_inactive", "chain.both_inactive_mask"]
    for g in ("plain", "count", "masked", "chain"):
        folded = g in ("masked", "chain")
        names = ["tx", "txaw", "txsw", "ax0", "ax1"] + (["mk0", "mk1"] if folded else [])
        R += ["%s.bp.%s.%s" % (g, n, p) for n in names
              for p in ("on16", "inside", "multi", "tail", "off")]
        R += ["%s.hang.area.%s" % (g, s) for s in "lrtb"]
        if folded:   # center_mask leaves a target that hangs off the image alone
            R += ["%s.hang.target.%s" % (g, s) for s in "lrtb"]
            R += [g + ".rows.ty_neg", g + ".rows.ty_over"]
            R += [g + ".degen.mask_inv", g + ".degen.mask_all", g + ".degen.no_mask"]
        R += [g + ".overlap.partial", g + ".overlap.disjoint", g + ".overlap.equal"]
        R += [g + ".rows.cross8", g + ".rows.cross32", g + ".rows.h_lt8"]
        R += ["%s.degen.%s" % (g, d) for d in ("inv_x", "inv_y", "one_px", "out_l", "out_r",
                                                "out_t")]   # out_b: see the table
    R += ["inplace.mask.narrow", "inplace.mask.inside", "inplace.mask.on16", "inplace.mask.tail"]
    for c in ("count", "dry"):
        R += ["%s.thr.%d" % (c, t) for t in THRESHOLDS]
        R += ["%s.cols.%s" % (c, k) for k in ("full", "single", "one_vector", "on16")]
        R.append(c + ".inactive")
    R += ["dry.ranges.aligned", "dry.ranges.unaligned", "dry.ranges.one_empty",
          "dry.only.none", "dry.only.0", "dry.only.1"]
    return R


# --------------------------------------------------------------- the table
G = (97, 61)
FULL = {(w, h): (0, 0, w - 1, h - 1) for (w, h) in SIZES}

# Single moves whose target lies inside the image, so that they serve as a
# centring too: (tag, size, area, tx, ty, a mask containing the area, classes)
_S = [
    # every breakpoint on a 16-multiple; source and target disjoint
    ("on16", G, (32, 8, 63, 23), 48, 30, (16, 2, 79, 50),
     ["bp.tx.on16", "bp.txsw.on16", "bp.ax0.on16", "bp.ax1.on16", "bp.mk0.on16",
      "bp.mk1.on16", "overlap.disjoint"]),
    # the area hangs off the left: tx + aw on a 16-multiple, the rest inside vectors
    ("hang_l", G, (-8, 4, 23, 19), 8, 30, (-9, 2, 70, 50),
     ["bp.txaw.on16", "bp.tx.inside", "bp.txsw.inside", "bp.ax0.off", "bp.ax1.inside",
      "hang.area.l", "bp.mk0.off", "bp.mk1.inside"]),
    # off the right
    ("hang_r", G, (70, 30, 110, 50), 6, 3, (13, 2, 96, 58),
     ["bp.txaw.inside", "bp.ax0.inside", "bp.ax1.off", "hang.area.r", "bp.mk0.inside",
      "bp.mk1.off"]),
    # off the top and the bottom: fewer rows copied than the target holds
    ("hang_t", G, (20, -6, 50, 10), 37, 40, None, ["hang.area.t"]),
    ("hang_b", G, (20, 50, 50, 70), 11, 10, (20, 40, 60, 60), ["hang.area.b"]),
    # a 3-wide area: four breakpoints in one vector, with a narrow mask six
    ("narrow", G, (35, 10, 37, 12), 41, 14, (33, 8, 39, 14),
     ["bp.tx.multi", "bp.txsw.multi", "bp.ax0.multi", "bp.ax1.multi", "bp.mk0.multi",
      "bp.mk1.multi"]),
    ("narrow_hang", G, (-2, 3, 2, 9), 20, 30, None, ["bp.txaw.multi"]),
    # the whole width moved down: every breakpoint at 0 or W
    ("full_width", G, (0, 5, 96, 20), 0, 30, (-5, -5, 200, 200),
     ["bp.tx.off", "bp.txsw.off", "bp.ax0.off", "bp.ax1.off", "bp.mk0.off", "bp.mk1.off",
      "degen.mask_all"]),
    # overlaps
    ("overlap_3x3", G, (20, 10, 50, 30), 48, 28, (18, 8, 52, 32), ["overlap.partial"]),
    ("overlap_col", G, (20, 10, 50, 30), 49, 12, None, ["overlap.partial"]),
    ("identity", G, (20, 10, 50, 30), 20, 10, (20, 10, 50, 30), ["overlap.equal"]),
    # rows
    ("cross8", G, (30, 5, 70, 10), 12, 40, None, ["rows.cross8"]),
    ("cross32", G, (30, 28, 70, 36), 12, 2, (30, 28, 70, 36), ["rows.cross32"]),
    ("cross32_48", (48, 33), (5, 25, 40, 32), 9, 0, (2, 20, 44, 32), ["rows.cross32"]),
    ("vertical_16", (16, 8), (0, 0, 15, 3), 0, 4, None, ["bp.tx.off"]),
    ("inner_16", (16, 8), (3, 1, 9, 5), 6, 2, (1, 0, 12, 6), ["bp.tx.inside"]),
    ("tail_7", (7, 5), (-1, 1, 1, 2), 3, 2, None,
     ["bp.tx.tail", "bp.txaw.tail", "bp.txsw.tail", "bp.ax1.tail", "rows.h_lt8"]),
    ("tail_7b", (7, 5), (4, 0, 5, 1), 1, 3, (3, 0, 5, 4),
     ["bp.ax0.tail", "bp.ax1.tail", "bp.mk0.tail", "bp.mk1.tail", "rows.h_lt8"]),
    ("tail_1043", (1043, 40), (100, 3, 140, 20), 1001, 15, (90, 1, 1040, 30),
     ["bp.txsw.tail", "bp.mk1.tail"]),
    # degenerate areas
    ("inv_x", G, (60, 10, 20, 30), 33, 25, (62, 32, 18, 8), ["degen.inv_x", "degen.mask_inv"]),
    ("inv_y", G, (20, 30, 60, 10), 3, 35, None, ["degen.inv_y"]),
    ("inv_xy", G, (75, 44, 41, 12), 7, 1, None, ["degen.inv_x", "degen.inv_y"]),
    ("one_px", G, (40, 20, 40, 20), 70, 50, (39, 19, 41, 21), ["degen.one_px"]),
    ("one_px_16", (16, 8), (15, 7, 15, 7), 0, 0, None, ["degen.one_px"]),
    ("out_l", G, (-20, 5, -10, 15), 3, 30, None, ["degen.out_l", "bp.txaw.off"]),
    ("out_r", G, (100, 5, 110, 15), 50, 30, None, ["degen.out_r"]),
    ("out_t", G, (10, -15, 30, -5), 40, 20, None, ["degen.out_t"]),
    # No area wholly below the image: it clips to y0 >= H, and k_move_rect_g16's
    # deferred vectors load their moved halves from row clip(area).y0 whether a
    # byte of them is used or not -- a row past the plane.  The table leaves
    # the geometry out until the kernel keeps that row inside.
]
# Targets that hang off the image: the align move only
_T = [
    ("target_l", G, (30, 20, 60, 40), -10, 5, None, ["hang.target.l"]),
    ("target_r", G, (30, 20, 60, 40), 80, 33, (30, 20, 60, 40), ["hang.target.r"]),
    ("target_t", G, (30, 20, 60, 40), 12, -7, (28, 18, 62, 42), ["hang.target.t", "rows.ty_neg"]),
    ("target_b", G, (30, 20, 60, 40), 50, 50, None, ["hang.target.b", "rows.ty_over"]),
    ("target_lt", (48, 33), (10, 8, 40, 30), -13, -5, None, ["hang.target.l", "hang.target.t"]),
    ("target_rb", (48, 33), (10, 8, 40, 30), 30, 20, (0, 0, 47, 32),
     ["hang.target.r", "hang.target.b", "degen.mask_all"]),
    ("target_7", (7, 5), (1, 1, 4, 3), 5, 3, None, ["hang.target.r", "rows.h_lt8"]),
]
_FAMILY_OF = {"inv": "degenerate", "one": "degenerate", "out": "degenerate", "cro": "rows",
              "ver": "rows", "tar": "rows", "han": "rows"}


def _family(tag):
    return _FAMILY_OF.get(tag[:3], "breakpoints")


def _single_cases():
    out = []
    n = 0
    for tag, size, area, tx, ty, mask, cl in _S + _T:
        hangs = (tag, size, area, tx, ty, mask, cl) in _T
        ident = "the move is the identity" if tag == "identity" else None
        for g, route in (("plain", PLAIN), ("count", COUNT), ("masked", MASKED)):
            n += 1
            own = [g + "." + c for c in cl if g == "masked" or not (
                c.startswith("bp.mk") or c.startswith("degen.mask"))]
            if route == MASKED:
                out.append(Case(_family(tag), tag, size, route, mask=mask, seed=n, classes=own,
                                align=align_to(area, tx, ty, ("lt", "rb", "c")[n % 3],
                                               force=ident is not None),
                                identity=ident if mask is None else None))
            elif not hangs:
                w = size[0]
                out.append(Case(_family(tag), tag, size, route, seed=n, classes=own,
                                center=center_to(area, tx, ty, force=ident is not None),
                                thr=THRESHOLDS[n % 5], identity=ident,
                                rx=[(0, w - 1), (w // 3, w // 3), (w // 2, w - 1)][n % 3]))
    return out


def _realign_cases():
    out = []
    for g, route in (("plain", PLAIN), ("count", COUNT), ("masked", MASKED)):
        for r in range(16):
            for on in (True, False):
                size = G if (r + on) % 4 else (97, 100)
                ax0 = 16 if on else 21
                area = (ax0, 9, ax0 + 47, 40)          # 48 wide: two whole vectors at least
                tx = ax0 - r + (32 if r % 2 and ax0 - r + 32 + 48 <= 97 else 0)
                ty = 2 + r
                seed = 100 + 32 * route + 2 * r + on
                cl = ["%s.realign.%d.%s" % (g, r, "on" if on else "off")]
                tag = "r%d_%s" % (r, "on" if on else "off")
                if route == MASKED:
                    mask = (ax0 - 3, 5, ax0 + 49, 44) if r % 2 == 0 else None
                    out.append(Case("realignment", tag, size, route, mask=mask, seed=seed,
                                    align=align_to(area, tx, ty, ("lt", "rb", "c")[r % 3]),
                                    classes=cl))
                else:
                    out.append(Case("realignment", tag, size, route, seed=seed, classes=cl,
                                    center=center_to(area, tx, ty), thr=THRESHOLDS[r % 5],
                                    rx=(r, 96 - 2 * r)))
    # the second 3072-column chunk: a 1401-wide block moved across it
    for g, route in (("plain", PLAIN), ("count", COUNT), ("masked", MASKED)):
        area, tx, ty = (100, 2, 1500, 30), 1688, 1    # to the last whole vector's end
        if route == MASKED:
            out.append(Case("realignment", "chunk2", (3089, 34), route, seed=7,
                            mask=(90, 0, 3081, 31), align=align_to(area, tx, ty, "rb"),
                            classes=[g + ".chunk2", g + ".realign.12.off"]))
        else:
            out.append(Case("realignment", "chunk2", (3089, 34), route, seed=8,
                            center=center_to(area, tx, ty), rx=(5, 3085),
                            classes=[g + ".chunk2", g + ".realign.12.off"]))
    return out


def _inplace_cases():
    """The align move inactive: the mask is applied in place."""
    masks = [
        ("narrow5", G, (40, 10, 44, 50), ["inplace.mask.narrow", "inplace.mask.inside"]),
        ("narrow1", G, (33, 0, 33, 60), ["inplace.mask.narrow"]),
        ("narrow15", (48, 33), (17, 30, 31, 32), ["inplace.mask.narrow", "inplace.mask.on16"]),
        ("on16", G, (32, 8, 63, 39), ["inplace.mask.on16"]),
        ("inside", G, (13, 2, 70, 50), ["inplace.mask.inside"]),
        ("inverted", G, (70, 50, 13, 2), ["masked.degen.mask_inv"]),
        ("outside", G, (120, 70, 130, 80), []),
        ("tail_7", (7, 5), (2, 1, 5, 3), ["inplace.mask.tail"]),
        ("tail_1043", (1043, 40), (5, 2, 1041, 30), ["inplace.mask.tail"]),
        ("wide_3089", (3089, 34), (3075, 1, 3086, 32), ["inplace.mask.narrow"]),
        ("one_16", (16, 8), (4, 2, 11, 5), ["inplace.mask.inside"]),
    ]
    out = [Case("degenerate", "inplace_" + t, size, MASKED, mask=m, seed=40 + i, classes=cl)
           for i, (t, size, m, cl) in enumerate(masks)]
    out.append(Case("degenerate", "inplace_all", G, MASKED, mask=FULL[G], seed=60,
                    classes=["masked.degen.mask_all"],
                    identity="a mask covering the image, no move"))
    out.append(Case("degenerate", "nothing", G, MASKED, seed=61, classes=["masked.degen.no_mask"],
                    identity="no mask, no move"))
    return out


# partners of the single moves in a chain
_CENTER = {G: ((10, 12, 50, 45), 14, 8), (48, 33): ((6, 4, 30, 20), 11, 9),
           (16, 8): ((2, 1, 8, 4), 5, 3), (7, 5): ((0, 0, 2, 1), 3, 2),
           (1043, 40): ((30, 4, 900, 30), 101, 6), (97, 100): ((10, 12, 50, 45), 14, 8)}
_ALIGN = {G: ((8, 6, 80, 52), 13, 3), (48, 33): ((4, 3, 40, 28), 7, 1),
          (16, 8): ((1, 1, 12, 6), 3, 0), (7, 5): ((1, 0, 5, 3), 0, 1),
          (1043, 40): ((40, 2, 1000, 35), 21, 4), (97, 100): ((8, 6, 80, 52), 13, 3)}


def _chain_cases():
    out = []
    n = 0
    # every single move as the chain's align move behind a plain centring, and
    # as its centring in front of a plain align move
    for tag, size, area, tx, ty, mask, cl in _S + _T:
        hangs = (tag, size, area, tx, ty, mask, cl) in _T
        ident = tag == "identity"
        n += 1
        own = ["chain." + c for c in cl]
        ca, ctx, cty = _CENTER[size]
        out.append(Case("chain", tag + "_align", size, CHAIN, seed=200 + n, mask=mask,
                        center=center_to(ca, ctx, cty), classes=own,
                        align=align_to(area, tx, ty, ("lt", "rb", "c")[n % 3], force=ident),
                        thr=THRESHOLDS[n % 5]))
        if not hangs:
            aa, atx, aty = _ALIGN[size]
            own = [c for c in own if ".bp.mk" not in c and ".degen.mask" not in c]
            out.append(Case("chain", tag + "_center", size, CHAIN, seed=300 + n,
                            center=center_to(area, tx, ty, force=ident), classes=own,
                            mask=None if n % 2 else normalize(aa),
                            align=align_to(aa, atx, aty, ("lt", "rb", "c")[n % 3]),
                            thr=THRESHOLDS[(n + 2) % 5]))
    # the combined offset: both moves shift a block that stays whole
    for r in range(16):
        r1 = (5 * r + 3) % 16
        r2 = (r - r1) % 16
        ca = (16, 10, 79, 50)                                # 64 wide
        ctx, cty = 16 - r1, 4
        aa = (ctx, 4, ctx + 63, 44)                          # the centred block
        atx, aty = ctx - r2 + (16 if ctx - r2 < 0 else 0), 9
        cl = ["chain.realign.%d" % r]
        if (r1 - r2) % 16:
            cl.append("chain.realign.differ")
        out.append(Case("chain", "combined_%d" % r, G, CHAIN, seed=400 + r,
                        center=center_to(ca, ctx, cty), mask=aa if r % 2 else None,
                        align=align_to(aa, atx, aty, ("lt", "rb", "c")[r % 3]), classes=cl))
    # the second lane pass holds one whole vector (columns 1024..1039): its
    # realignment is the wave's
    for r in range(16):
        ca = (500 + r, 3, 560 + r, 30)                       # 61 wide
        ctx, cty = 980, 6                                    # columns 980..1040
        out.append(Case("chain", "pass2_%d" % r, (1043, 40), CHAIN, seed=500 + r,
                        center=center_to(ca, ctx, cty), rx=(1000, 1042),
                        mask=None if r % 3 else (3, 1, 1041, 38),
                        classes=["chain.uniform.%d" % ((500 + r - 980) % 16), "chain.pass2"]))
    extra = [
        # the moves and the mask switched off in turn
        ("center_inactive", G, None, ((30, 20, 60, 40), 44, 11), (28, 18, 62, 42),
         ["chain.center_inactive"], None),
        ("align_inactive", G, ((10, 12, 50, 45), 31, 8), None, (13, 2, 70, 50),
         ["chain.align_inactive"], None),
        ("align_inactive_nomask", G, ((10, 12, 50, 45), 31, 8), None, None,
         ["chain.align_inactive", "chain.degen.no_mask"], None),
        ("mask_only", G, None, None, (13, 2, 70, 50), ["chain.both_inactive_mask"], None),
        ("mask_only_7", (7, 5), None, None, (2, 1, 5, 3), ["chain.both_inactive_mask"], None),
        ("copy", (48, 33), None, None, None, [], "no move, no mask: the chain copies the page"),
        # exactly three breakpoints in a vector: 35, 37, 46 (48 lies on its edge)
        ("three_bp", G, ((35, 10, 36, 40), 46, 12), None, None, ["chain.bytes.three_bp"], None),
        # six of them: a 3-wide area, a 7-wide mask
        ("many_bp", G, None, ((35, 10, 37, 12), 41, 14), (33, 8, 39, 14),
         ["chain.bytes.many_bp"], None),
        # the target in the first block of rows, the area in the second: each
        # block drops the other's breakpoints
        ("live_drop", G, None, ((40, 40, 70, 55), 8, 2), None, ["chain.live_drop"], None),
        ("live_drop_both", G, ((40, 40, 70, 55), 8, 2), ((5, 34, 40, 58), 50, 33), None,
         ["chain.live_drop"], None),
        ("one_vector", (16, 8), ((0, 0, 15, 3), 0, 4), ((0, 2, 15, 7), 0, 0), None,
         ["chain.uniform.0"], None),
    ]
    for i, (tag, size, c, a, mask, cl, ident) in enumerate(extra):
        out.append(Case("chain", tag, size, CHAIN, seed=600 + i, mask=mask, classes=cl,
                        center=center_to(*c) if c else None,
                        align=align_to(*a, ("c", "lt", "rb")[i % 3]) if a else None,
                        identity=ident, thr=THRESHOLDS[i % 5]))
    return out


def _count_cases():
    out = []
    move = ((20, 10, 70, 40), 33, 15)
    cols = {"full": (0, 96), "single": (37, 37), "one_vector": (34, 45), "on16": (16, 79)}
    n = 0
    for c, route in (("count", COUNT), ("dry", DRY)):
        for thr in THRESHOLDS:
            for k, rx in cols.items():
                n += 1
                out.append(Case("counts", "%s_thr%d" % (k, thr), G, route, seed=700 + n, rx=rx,
                                thr=thr, center=center_to(*move),
                                classes=["%s.thr.%d" % (c, thr), "%s.cols.%s" % (c, k)]))
        # no centring: the page's own rows are counted
        out.append(Case("counts", "inactive", G, route, seed=750 + route, rx=(3, 90), thr=127,
                        classes=[c + ".inactive"],
                        identity="no centring: the page's own rows are counted"))
        for size in ((7, 5), (16, 8), (48, 33), (1043, 40), (3089, 34)):
            w, h = size
            area = (w // 5, 1, w // 5 + w // 2, h - 2)
            out.append(Case("counts", "size", size, route, seed=760 + w + route, thr=170,
                            center=center_to(area, w // 3, 0), rx=(1, w - 2),
                            classes=[c + ".thr.170"]))
    big = (97, 100)
    dry = [
        ("unaligned", (0, 40, 61, 100), -1, ["dry.ranges.unaligned", "dry.only.none"]),
        ("aligned", (0, 32, 64, 96), -1, ["dry.ranges.aligned"]),
        ("second_empty", (10, 50, 0, 0), -1, ["dry.ranges.one_empty"]),
        ("first_empty", (0, 0, 61, 100), 1, ["dry.ranges.one_empty", "dry.only.1"]),
        ("only_0", (0, 0, 0, 0), 0, ["dry.only.0"]),
        ("only_0_ranges", (0, 40, 61, 100), 0, ["dry.only.0"]),
        ("only_1", (0, 0, 0, 0), 1, ["dry.only.1"]),
    ]
    for i, (tag, ranges, only, cl) in enumerate(dry):
        out.append(Case("counts", tag, big, DRY, seed=800 + i, ranges=ranges, only=only,
                        center=center_to((20, 10, 70, 90), 9, 3), rx=(5, 91), thr=170,
                        classes=cl))
        out.append(Case("counts", tag, big, CHAIN, seed=820 + i, ranges=ranges, only=only,
                        center=center_to((20, 10, 70, 90), 9, 3), rx=(5, 91), thr=127,
                        mask=(4, 2, 80, 96), align=align_to((9, 3, 59, 83), 30, 10, "c"),
                        classes=cl))
    return out


_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        _CASES = (_realign_cases() + _single_cases() + _inplace_cases() + _chain_cases() +
                  _count_cases())
    return _CASES


def family_cases(family):
    return [c for c in all_cases() if c.family == family]
