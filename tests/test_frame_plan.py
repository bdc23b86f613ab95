"""The frame planner (csrc/frame_plan.cpp), the host-only half of the frame driver, on the CPU: the film's pixel layout, the pixel cap of a
frame, the batch cutter and the pass schedule against restatements in plain Python integers, case by case and exactly.
tests/native/host_frame_plan.cpp wraps the planner for ctypes; the same source is a stand-alone program for a run under AddressSanitizer /
UBSan.  Nothing here reads the C++."""
import ctypes as C
import itertools

import pytest

import adaptive64
import frame_cases
import native_lib as NL
from native_lib import ERR_ARG
from phosphorus_mk2_amd import abi

M = 1 << 20
NONE = 0xffffffff  # no back-off limit
AMPLE = 1 << 40


# ---- the rules, restated ----------------------------------------------------------------------------------------------------------------
def model_layout(pc, normals, moments, adaptive):
    """-> (xstride, normals_offset, m2_offset, samples_offset, path_bytes)"""
    xstride = pc + 3 * normals + 3 * moments + adaptive
    path_bytes = (192 if normals else 176) + 12 * moments
    if adaptive:
        path_bytes += 4 + 4 * xstride + 12
    return xstride, pc if normals else 0, pc + 3 * normals, xstride - 1, path_bytes


def model_cap(budget, spp, flight=0, adaptive=None):
    """adaptive: (min_samples, step) or None"""
    frame_samples = min(spp, max(adaptive)) if adaptive else spp
    pass_samples = max(1, min(spp, flight or frame_samples))
    return min(8 * M, max(budget // pass_samples, 64 << 10))


def model_passes(P, spp, flight, budget, adaptive=None, limit=NONE):
    """-> (S, [(s0, ns, round_end)])"""
    def split(r):  # samples per pass of a round of r samples
        if flight:
            return flight
        smax = max(1, min(max(budget, P) // P, 0x7ffffff0 // P))
        npasses = -(-r // smax)
        return -(-r // npasses)
    ends = [spp]
    if adaptive:
        ends = [min(adaptive[0], spp)]
        while ends[-1] < spp:
            ends.append(min(ends[-1] + adaptive[1], spp))
    out, S, begin = [], 0, 0
    for end in ends:
        Sr = min(split(end - begin), end - begin, limit)
        for s0 in range(begin, end, Sr):
            out.append((s0, min(Sr, end - s0), int(bool(adaptive) and s0 + Sr >= end)))
        S = max(S, Sr)
        begin = end
    return S, out


def morton(tile):
    def spread(v):
        return sum(((v >> b) & 1) << (2 * b) for b in range(16))
    return spread(tile[0] >> 5) | (spread(tile[1] >> 5) << 1)


def model_cut(tiles, cap, tiles_per_batch, W, H):
    """-> the batches, each in Morton order (Python's sort is stable), or None when a tile is refused"""
    batches, cur, px = [], [], 0
    for t in tiles:
        x, y, w, h = t
        if w == 0 or h == 0 or x + w > W or y + h > H:
            return None
        if cur and ((tiles_per_batch and len(cur) == tiles_per_batch) or px >= cap or px + w * h > cap):
            batches.append(cur)
            cur, px = [], 0
        cur.append(t); px += w * h
    if cur:
        batches.append(cur)
    return [sorted(b, key=morton) for b in batches]


def grid(W, H, ts=32):
    return [(x, y, min(ts, W - x), min(ts, H - y)) for y in range(0, H, ts) for x in range(0, W, ts)]


# ---- the library ---------------------------------------------------------------------------------------------------------------------------
class Planner:
    def __init__(self, lib):
        self.lib = lib
        lib.fp_layout.restype = None; lib.fp_layout.argtypes = [C.c_uint32] * 4 + [C.POINTER(C.c_uint64)]
        lib.fp_pixel_cap.restype = C.c_uint64; lib.fp_pixel_cap.argtypes = [C.c_uint64] + [C.c_uint32] * 4
        lib.fp_passes.restype = C.c_uint32
        lib.fp_passes.argtypes = [C.c_uint32] * 3 + [C.c_uint64] + [C.c_uint32] * 3 + [abi.u32p, C.c_uint32, abi.u32p]
        lib.fp_cut.restype = C.c_int
        lib.fp_cut.argtypes = [C.POINTER(abi.Tile), C.c_uint32, C.c_uint64] + [C.c_uint32] * 3 + [C.POINTER(abi.Tile), abi.u32p, abi.u32p, C.c_char_p, C.c_uint32]

    def layout(self, pc, normals, moments, adaptive):
        out = (C.c_uint64 * 5)()
        self.lib.fp_layout(pc, normals, moments, adaptive, out)
        return tuple(out)

    def cap(self, budget, spp, flight=0, adaptive=None):
        return self.lib.fp_pixel_cap(budget, spp, flight, *(adaptive or (0, 0)))

    def passes(self, P, spp, flight, budget, adaptive=None, limit=NONE):
        room = spp  # a pass carries at least one sample
        out, S = (C.c_uint32 * (3 * room))(), C.c_uint32(0)
        n = self.lib.fp_passes(P, spp, flight, budget, *(adaptive or (0, 0)), limit, out, room, C.byref(S))
        assert n <= room
        return S.value, [tuple(out[3 * i:3 * i + 3]) for i in range(n)]

    def cut(self, tiles, cap, tiles_per_batch, W, H):
        """-> (status, batches, message)"""
        n = len(tiles)
        src, dst = (abi.Tile * n)(*[abi.Tile(*t) for t in tiles]), (abi.Tile * n)()
        sizes, nb, err = (C.c_uint32 * n)(), C.c_uint32(0), C.create_string_buffer(64)
        rc = self.lib.fp_cut(src, n, cap, tiles_per_batch, W, H, dst, sizes, C.byref(nb), err, len(err))
        flat = [(t.x, t.y, t.w, t.h) for t in dst]
        starts = [sum(sizes[:b]) for b in range(nb.value + 1)]
        return rc, [flat[starts[b]:starts[b + 1]] for b in range(nb.value)], err.value.decode()


@pytest.fixture(scope="module")
def plan():
    """the host_frame_plan library behind a Planner"""
    return Planner(NL.load("host_frame_plan"))


# ---- 1. the film's pixel layout ----------------------------------------------------------------------------------------------------------
LAYOUTS = [(pc, normals, moments, adaptive) for pc in (3, 4) for normals in (0, 1) for moments, adaptive in ((0, 0), (1, 0), (1, 1))]


@pytest.mark.parametrize("case", LAYOUTS, ids=["pc%d_n%d_m%d_a%d" % c for c in LAYOUTS])
def test_layout(plan, case):
    assert plan.layout(*case) == model_layout(*case)


def test_layout_figures(plan):
    assert plan.layout(4, 0, 0, 0) == (4, 0, 4, 3, 176)
    assert plan.layout(3, 1, 0, 0) == (6, 3, 6, 5, 192)
    assert plan.layout(4, 1, 1, 0) == (10, 4, 7, 9, 192 + 12)
    assert plan.layout(4, 1, 1, 1) == (11, 4, 7, 10, 192 + 12 + 4 + 44 + 12)
    assert plan.layout(3, 0, 1, 1) == (7, 0, 3, 6, 176 + 12 + 4 + 28 + 12)


# ---- 2. the pixel cap ------------------------------------------------------------------------------------------------------------------------
CAPS = [((512 * M, 16), 8 * M), ((512 * M, 256), 2 * M), ((512 * M, 4096), 131072), ((512 * M, 65536), 65536),
        ((512 * M, 256, 32), 8 * M), ((512 * M, 256, 0, (16, 16)), 8 * M), ((512 * M, 256, 0, (300, 16)), 512 * M // 256)]


@pytest.mark.parametrize("args,want", CAPS, ids=[str(i) for i in range(len(CAPS))])
def test_pixel_cap(plan, args, want):
    assert plan.cap(*args) == want == model_cap(*args)


# ---- 3. the pass schedule without adaptive sampling -----------------------------------------------------------------------------------------
def sizes(passes):
    return [ns for _, ns, _ in passes]


def covers(passes, spp):
    """every sample 0 .. spp - 1 exactly once, in order"""
    return [s for s0, ns, _ in passes for s in range(s0, s0 + ns)] == list(range(spp))


UNIFORM = [((1024, 16, 0, 10000), [8, 8]), ((1024, 20, 0, 10000), [7, 7, 6]), ((1024, 256, 0, 10000), [9] * 28 + [4]),
           ((1024, 16, 0, 10000, None, 4), [4, 4, 4, 4]), ((1024, 5, 0, 10), [1] * 5), ((1024, 8, 3, 10000), [3, 3, 2]), ((1024, 2, 3, 10000), [2])]


@pytest.mark.parametrize("args,want", UNIFORM, ids=[str(i) for i in range(len(UNIFORM))])
def test_pass_schedule(plan, args, want):
    S, passes = plan.passes(*args)
    assert sizes(passes) == want and S == max(want)
    assert covers(passes, args[1]) and not any(re for _, _, re in passes)
    assert (S, passes) == model_passes(*args)


def test_samples_in_flight_ignores_the_budget(plan):
    for budget in (0, 10, 10000, AMPLE):
        assert plan.passes(1024, 8, 3, budget) == (3, [(0, 3, 0), (3, 3, 0), (6, 2, 0)])


def test_paths_of_a_pass_stay_below_2_to_the_31(plan):
    P, spp = 3 * M, 4096
    S, passes = plan.passes(P, spp, 0, 1 << 62)
    smax = 0x7ffffff0 // P
    assert smax == 682 and (smax + 1) * P > 0x7ffffff0
    assert len(passes) == 7 == -(-spp // smax) and -(-spp // 6) > smax  # the fewest passes of at most smax samples ...
    assert S == 586 == -(-spp // 7) and sizes(passes) == [586] * 6 + [580] and S * P < 1 << 31  # ... made equal
    assert covers(passes, spp) and (S, passes) == model_passes(P, spp, 0, 1 << 62)


# ---- 4. the pass schedule with adaptive sampling ----------------------------------------------------------------------------------------------
def test_adaptive_rounds(plan):
    S, passes = plan.passes(1024, 16, 0, AMPLE, (4, 5))
    assert passes == [(0, 4, 1), (4, 5, 1), (9, 5, 1), (14, 2, 1)] and S == 5
    S, passes = plan.passes(1024, 16, 3, AMPLE, (4, 5))
    assert sizes(passes) == [3, 1, 3, 2, 3, 2, 2] and [re for _, _, re in passes] == [0, 1, 0, 1, 0, 1, 1] and S == 3
    assert covers(passes, 16)


def test_adaptive_edges(plan):
    for min_samples in (16, 17, 40, NONE):  # min_samples >= spp: one round
        assert plan.passes(1024, 16, 0, AMPLE, (min_samples, 5)) == (16, [(0, 16, 1)])
    for step in (13, 1000, NONE):  # the first increment is clamped to spp
        assert plan.passes(1024, 16, 0, AMPLE, (4, step)) == (12, [(0, 4, 1), (4, 12, 1)])
    # a budget that splits the rounds, and the back-off's limit on top
    assert plan.passes(1024, 16, 0, 10000, (4, 5), 2) == model_passes(1024, 16, 0, 10000, (4, 5), 2)
    assert sizes(plan.passes(1024, 16, 0, 10000, (4, 5), 2)[1]) == [2, 2, 2, 2, 1, 2, 2, 1, 2]


def test_adaptive_schedule_is_the_one_of_adaptive64(plan):
    for spp, min_samples, step, flight in itertools.product(range(1, 21), range(2, 7), range(1, 6), range(0, 5)):
        S, passes = plan.passes(64, spp, flight, AMPLE, (min_samples, step))
        ends = adaptive64.round_ends(spp, min_samples, step)
        assert [s0 + ns for s0, ns, re in passes if re] == ends, (spp, min_samples, step, flight)
        want = [ns for begin, end in zip([0] + ends, ends) for ns in adaptive64.round_passes(end - begin, flight)]
        assert sizes(passes) == want and covers(passes, spp) and S == max(want), (spp, min_samples, step, flight)
        assert (S, passes) == model_passes(64, spp, flight, AMPLE, (min_samples, step))


# ---- 5. the batch cutter -----------------------------------------------------------------------------------------------------------------------
W, H = 320, 200
TILES = grid(W, H)


def px(batch):
    return sum(w * h for _, _, w, h in batch)


def test_the_film_of_the_cases():
    assert len(TILES) == 70 and TILES[-1] == (288, 192, 32, 8) and px(TILES) == W * H


@pytest.mark.parametrize("cap,tiles_per_batch", [(65536, 0), (4096, 0), (65536, 3), (100, 0), (4096, 3), (1024, 0), (1025, 0)])
def test_batches(plan, cap, tiles_per_batch):
    rc, batches, err = plan.cut(TILES, cap, tiles_per_batch, W, H)
    assert rc == 0 and err == ""
    assert batches == model_cut(TILES, cap, tiles_per_batch, W, H)
    assert sorted(t for b in batches for t in b) == sorted(TILES)  # every tile once
    # each batch is a run of the queue, in Morton order
    k = 0
    for b in batches:
        assert b == sorted(TILES[k:k + len(b)], key=morton)
        k += len(b)
    for i, b in enumerate(batches):
        assert len(b) == 1 or px(b) <= cap  # never above the cap, but for a lone tile
        assert not tiles_per_batch or len(b) <= tiles_per_batch
        if i + 1 < len(batches):  # it ended because it was full: by count, or the queue's next tile — which opens the next batch — would overflow
            nxt = TILES[sum(len(x) for x in batches[:i + 1])]
            assert nxt in batches[i + 1] and (len(b) == tiles_per_batch or px(b) + nxt[2] * nxt[3] > cap)


def test_batch_figures(plan):
    assert [len(b) for b in plan.cut(TILES, 65536, 0, W, H)[1]] == [70]
    assert [len(b) for b in plan.cut(TILES, 65536, 3, W, H)[1]] == [3] * 23 + [1]
    assert [len(b) for b in plan.cut(TILES, 100, 0, W, H)[1]] == [1] * 70
    by_cap = plan.cut(TILES, 4096, 0, W, H)[1]
    assert [len(b) for b in by_cap[:15]] == [4] * 15 and max(px(b) for b in by_cap) == 4096  # whole tiles: 4 x 1 024; the edge row packs closer
    assert px(by_cap[-1]) <= 4096 and sum(len(b) for b in by_cap) == 70


@pytest.mark.parametrize("tiles", [frame_cases.strip_tiles(67, 5), [(x, 0, 1, 5) for x in (40, 3, 33, 0, 63, 31, 32, 5, 64)]], ids=["strips_67x5", "columns"])
@pytest.mark.parametrize("cap", [65536, 80])
def test_tiles_with_equal_keys_keep_their_order(plan, tiles, cap):
    assert len({morton(t) for t in tiles}) < len(tiles)
    rc, batches, _ = plan.cut(tiles, cap, 0, 67, 5)
    assert rc == 0 and batches == model_cut(tiles, cap, 0, 67, 5)
    for b in batches:
        for key in {morton(t) for t in b}:
            assert [t for t in b if morton(t) == key] == [t for t in tiles if morton(t) == key and t in b]


@pytest.mark.parametrize("bad", [(288, 192, 0, 8), (288, 192, 32, 0), (289, 192, 32, 8), (288, 193, 32, 8), (0xffffffff, 0, 2, 1), (0, 0xffffffff, 1, 2)],
                         ids=["no_width", "no_height", "past_the_right_edge", "past_the_bottom_edge", "x_wraps", "y_wraps"])
@pytest.mark.parametrize("where", [0, 35, 69])
def test_a_tile_outside_the_film_is_refused(plan, bad, where):
    tiles = list(TILES); tiles[where] = bad
    assert model_cut(tiles, 65536, 0, W, H) is None
    for cap, tiles_per_batch in ((65536, 0), (4096, 0), (65536, 1)):
        rc, _, err = plan.cut(tiles, cap, tiles_per_batch, W, H)
        assert rc == ERR_ARG and err == "tile outside the film"


# ---- 6. under AddressSanitizer and UBSan, stand-alone --------------------------------------------------------------------------------------
def check_line(line):
    """one line of the program's output, "<what> <the case> : <what the planner decided>", against the models"""
    case, _, got = line.partition(" : ")
    what, *args = case.split()
    if what == "cut":
        name, (cap, tiles_per_batch, w, h) = args[0], map(int, args[1:])
        tiles = frame_cases.strip_tiles(w, h) if name == "strips" else grid(w, h)
        if name != "grid" and name != "strips":
            x, y, tw, th = tiles[-1]
            tiles[-1] = {"empty": (x, y, 0, th), "right": (x + 1, y, tw, th), "bottom": (x, y + 1, tw, th)}[name]
        want = model_cut(tiles, cap, tiles_per_batch, w, h)
        if want is None:
            return got == "1 tile outside the film"
        return got == " ".join(["0"] + ["| " + " ".join("%d,%d,%d,%d" % t for t in b) for b in want])
    args = [int(a) for a in args]
    if what == "layout":
        want = model_layout(*args)
    elif what == "cap":
        want = [model_cap(args[0], args[1], args[2], tuple(args[3:5]) if args[3] else None)]
    else:
        assert what == "passes"
        S, passes = model_passes(args[0], args[1], args[2], args[3], tuple(args[4:6]) if args[4] else None, args[6])
        want = [S] + [v for p in passes for v in p]
    return [int(v) for v in got.split()] == list(want)


def test_the_planner_under_the_sanitizers(tmp_path):
    """host_frame_plan.cpp's own main(): the cases of this file in exactly sized heap arrays, every decision printed; each line is checked
    against the models above, and the program ends without a report."""
    lines = NL.run_sanitized(tmp_path, "host_frame_plan", "HOST_FRAME_PLAN_MAIN").splitlines()
    assert [sum(l.startswith(w) for l in lines) for w in ("layout", "cap", "passes", "cut")] == [12, 7, 15, 9]
    for line in lines:
        assert check_line(line), line
