"""The tile map (phx_tile_map) without a GPU: the ABI and the header's text, every refusal of the argument check
(csrc/tile_map_check.cpp through tests/native/tile_map_host.cpp), the Python helpers, the float64 model of the rule (tests/tile_map64.py) on
hand-made films, and the progressive loop's pooling on the oracle's films.  The device is held to the same model bit for bit in
tests/test_gpu_tile_map.py."""
import ctypes as C
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import accumulate64 as ac
import frame_cases as FC
import native_lib as NL
import tile_map64 as tm
from conftest import bits_equal
from native_lib import CSRC, ERR_ARG, NATIVE

F, D = np.float32, np.float64

# the host library of this module: a registry of its own (folding it into native_lib.REGISTRY is a follow-up)
REGISTRY = {"tile_map_host": ([os.path.join(NATIVE, "tile_map_host.cpp"), os.path.join(CSRC, "tile_map_check.cpp")], [])}


# ---- 1. the ABI and the header ------------------------------------------------------------------------------------------------------------
FIELDS = ["width", "height", "xstride", "m2_offset", "samples_offset", "tile_width", "tile_height", "on_device", "tau", "floor", "reserved"]
RECORD_FIELDS = ["tile", "invalid", "starved", "converged", "worst", "samples"]
SUMMARY_FIELDS = ["pixels", "invalid", "converged", "samples", "tiles", "open"]


def test_struct_sizes_and_field_offsets():
    from phosphorus_mk2_amd import abi, xpu
    assert C.sizeof(abi.TileMap) == 56
    assert [f for f, _ in abi.TileMap._fields_] == FIELDS
    assert [getattr(abi.TileMap, f).offset for f in FIELDS] == [4 * i for i in range(11)]
    assert abi.TileMap.tau.size == 4 and abi.TileMap.floor.size == 4 and abi.TileMap.reserved.size == 16
    assert C.sizeof(abi.TileRecord) == 40 and [f for f, _ in abi.TileRecord._fields_] == RECORD_FIELDS
    assert [getattr(abi.TileRecord, f).offset for f in RECORD_FIELDS] == [0, 16, 20, 24, 28, 32]
    assert C.sizeof(abi.TileMapSummary) == 48 and [f for f, _ in abi.TileMapSummary._fields_] == SUMMARY_FIELDS
    assert [getattr(abi.TileMapSummary, f).offset for f in SUMMARY_FIELDS] == [8 * i for i in range(6)]
    for name in ("phx_dev_film_tile_map", "phx_dev_tile_map_times", "phx_tiles_make_list"):
        assert name in abi.EXPORTS
    # numpy's view of a record, the model's and the package's, is the struct
    for dt in (tm.RECORD, xpu.TILE_RECORD):
        assert dt.itemsize == 40 and [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 12, 16, 20, 24, 28, 32]
        assert dt.names == ("x", "y", "w", "h", "invalid", "starved", "converged", "worst", "samples")


def test_struct_sizes_are_the_librarys():
    from phosphorus_mk2_amd import abi, xpu
    if not os.path.exists(xpu.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = xpu.load_library()
    assert (lib.phx_abi_sizeof(25), lib.phx_abi_sizeof(26), lib.phx_abi_sizeof(27)) == (C.sizeof(abi.TileMap), C.sizeof(abi.TileRecord), C.sizeof(abi.TileMapSummary))
    assert lib.phx_abi_sizeof(18) == C.sizeof(abi.Accumulate) and lib.phx_abi_sizeof(24) == C.sizeof(abi.OutlierClampSummary)  # the earlier indices stay


def test_header_states_the_structs_and_the_rule():
    hdr, body = NL.header(), NL.struct_body("phx_tile_map", strip_comments=False)
    assert re.findall(r"\b(\w+)(?:\[4\])?[;,]", NL.struct_body("phx_tile_map")) == FIELDS
    assert re.search(r"uint32_t\s+width,\s*height;", body) and re.search(r"float\s+tau;", body) and re.search(r"float\s+floor;", body)
    assert re.search(r"uint32_t\s+tile_width,\s*tile_height;\s*/\* 4 \.\. 1024 each \*/", body)
    rec = NL.struct_body("phx_tile_record")
    assert re.search(r"phx_tile\s+tile;\s*uint32_t\s+invalid,\s*starved,\s*converged;\s*float\s+worst;\s*uint64_t\s+samples;", rec)
    assert re.search(r"uint64_t\s+pixels,\s*invalid,\s*converged,\s*samples,\s*tiles,\s*open;\s*\} phx_tile_map_summary;", hdr)
    assert re.search(r"int\s+phx_dev_film_tile_map\(phx_device\* dev, const phx_tile_map\* m, const float\* acc, phx_tile_record\* records, "
                     r"phx_tile_map_summary\* summary", hdr)
    assert re.search(r"int\s+phx_dev_tile_map_times\(const phx_device\* dev, double\* ms", hdr)
    assert re.search(r"phx_tiles\*\s+phx_tiles_make_list\(const phx_tile\* tiles, uint32_t count\);", hdr)
    rule = hdr[hdr.index("the tile map (DESIGN 26)"):hdr.index("typedef struct phx_tile_map")]
    flat = NL.flat(rule)
    for phrase in ["tx = ceil(width / tile_width)", "ty = ceil(height / tile_height)", "record j tx + i covers x in [i tile_width, min((i + 1) tile_width, width))",
                   "rows run top to bottom and tiles left to right", "phx_tiles_make(width, height, tile_size, 0, 1)", "in binary64, without contraction",
                   "all six floats finite, every m_c >= 0, n finite and n >= 2", "n finite and 0 <= n < 2, whatever the other floats hold",
                   "A starved pixel is also invalid", "q = n / (n - 1)", "L = m_c q", "den = fabs(V_c) + floor", "b = tau den", "ok_c = L <= b b",
                   "converged = ok_r && ok_g && ok_b", "r_c = den > 0 ? sqrt(L) / den : (L == 0 ? 0 : +inf)", "r = fp32(max(r_r, r_g, r_b))",
                   "it may round to +inf", "(uint64_t)min(n, 2^53)", "+0.0f when there are none", "does not depend on the reduction's order",
                   "OPEN when converged < w h - invalid or starved > 0", "Its first four fields equal phx_accumulate_summary of the same film"]:
        assert " ".join(phrase.split()) in flat, phrase


@pytest.mark.parametrize("pc", [3, 4])
@pytest.mark.parametrize("normals", [False, True])
def test_python_settings_are_the_accumulators_layout(pc, normals):
    from phosphorus_mk2_amd import xpu
    acc = xpu.accumulator(7, 5, pc, normals)
    q = xpu.tile_map_settings(acc.shape, 8, 0.05, 0.01, pc, normals)
    xs, _, mo, so = ac.layout(pc, normals, True)
    assert (q.width, q.height, q.xstride, q.m2_offset, q.samples_offset) == (7, 5, xs, mo, so)
    assert (q.tile_width, q.tile_height, q.on_device, q.tau, q.floor, list(q.reserved)) == (8, 8, 0, F(0.05), F(0.01), [0] * 4)
    q = xpu.tile_map_settings(acc.shape, (16, 4), 0.0, 0.0, pc, normals)
    assert (q.tile_width, q.tile_height) == (16, 4)
    with pytest.raises(ValueError, match="xpu.accumulator"):
        xpu.tile_map_settings((5, 7, xs - 1), 8, 0.05, 0.0, pc, normals)
    with pytest.raises(ValueError, match="height, width, xstride"):
        xpu.tile_map_settings((5, 7), 8)


def test_render_progressive_refuses_what_tiles_cannot_be_combined_with():
    """argument checks that come before any device is made"""
    from phosphorus_mk2_amd import scenes, xpu
    sc = scenes.cornell(32, 32)
    with pytest.raises(ValueError, match="despeckle"):
        next(xpu.render_progressive(sc, 4, 2, stop=dict(threshold=0.1), tiles=dict(size=8), despeckle={}))
    with pytest.raises(ValueError, match="stop"):
        next(xpu.render_progressive(sc, 4, 2, tiles=dict(size=8)))
    with pytest.raises(ValueError, match="does not know"):
        next(xpu.render_progressive(sc, 4, 2, stop=dict(threshold=0.1), tiles=dict(sizes=8)))
    with pytest.raises(ValueError, match="min_frames"):
        next(xpu.render_progressive(sc, 4, 2, stop=dict(threshold=0.1), tiles=dict(min_frames=0)))


# ---- 2. the refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    from phosphorus_mk2_amd import abi
    lib = NL.load("tile_map_host", registry=REGISTRY)
    for f in ("tm_sizeof", "tm_sizeof_record", "tm_sizeof_summary", "tm_tiles"):
        getattr(lib, f).restype = C.c_uint32
    lib.tm_tiles.argtypes = [C.c_uint32, C.c_uint32]
    assert (lib.tm_sizeof(), lib.tm_sizeof_record(), lib.tm_sizeof_summary()) == (C.sizeof(abi.TileMap), C.sizeof(abi.TileRecord), C.sizeof(abi.TileMapSummary))
    offs = (C.c_uint32 * 6)()
    lib.tm_record_offsets(offs)
    assert list(offs) == [getattr(abi.TileRecord, f).offset for f in RECORD_FIELDS]
    return lib


@pytest.fixture(scope="module")
def check(host):
    """(abi.TileMap, film address, records address) -> (status, message)"""
    from phosphorus_mk2_amd import abi
    tm_check = NL.checker(host, "tm_check", [C.POINTER(abi.TileMap), C.c_void_p, C.c_void_p])
    return lambda q, acc=0x10000, records=1 << 44: tm_check(C.byref(q), acc, records)  # (far apart: the largest film is 2^32 pixels of 96 bytes)


def good(**kw):
    from phosphorus_mk2_amd import abi
    q = abi.TileMap(width=64, height=48, xstride=11, m2_offset=7, samples_offset=10, tile_width=32, tile_height=16, on_device=0, tau=0.05, floor=0.01)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


ACCEPTED = [dict(), dict(width=1, height=1), dict(width=65536, height=65536), dict(on_device=1), dict(on_device=2), dict(tau=0.0, floor=0.0),
            dict(xstride=7, m2_offset=3, samples_offset=6), dict(xstride=7, m2_offset=4, samples_offset=3), dict(xstride=24, m2_offset=21, samples_offset=3),
            dict(xstride=24, m2_offset=3, samples_offset=23), dict(tile_width=4, tile_height=4), dict(tile_width=1024, tile_height=1024),
            dict(tile_width=4, tile_height=1024), dict(width=3, height=2, tile_width=64, tile_height=64)]
REFUSED = [("width", dict(width=0)), ("width", dict(width=65537)), ("height", dict(height=0)), ("height", dict(height=65537)),
           ("xstride", dict(xstride=6)), ("xstride", dict(xstride=25)), ("xstride", dict(xstride=0)),
           ("m2_offset", dict(m2_offset=0)), ("m2_offset", dict(m2_offset=2)), ("m2_offset", dict(m2_offset=9)), ("m2_offset", dict(m2_offset=0xfffffffe)),
           ("samples_offset", dict(samples_offset=0)), ("samples_offset", dict(samples_offset=2)), ("samples_offset", dict(samples_offset=11)),
           ("samples_offset", dict(samples_offset=8)), ("samples_offset", dict(samples_offset=0xffffffff)),
           ("tile_width", dict(tile_width=0)), ("tile_width", dict(tile_width=3)), ("tile_width", dict(tile_width=1025)),
           ("tile_height", dict(tile_height=0)), ("tile_height", dict(tile_height=3)), ("tile_height", dict(tile_height=1025)),
           ("on_device", dict(on_device=3)), ("on_device", dict(on_device=0xffffffff)),
           ("tau", dict(tau=-1.0)), ("tau", dict(tau=float("nan"))), ("tau", dict(tau=float("inf"))),
           ("floor", dict(floor=-1.0)), ("floor", dict(floor=float("nan"))), ("floor", dict(floor=float("inf")))]


@pytest.mark.parametrize("kw", ACCEPTED, ids=NL.case_ids(ACCEPTED))
def test_check_accepts(check, kw):
    assert check(good(**kw)) == (0, "")


@pytest.mark.parametrize("field,kw", REFUSED, ids=NL.case_ids(kw for _, kw in REFUSED))
def test_check_refuses_and_names_the_field(check, field, kw):
    rc, msg = check(good(**kw))
    assert rc == ERR_ARG and re.search(rf"\b{field}\b", msg) and msg.startswith("tile_map: ") and msg.endswith("(phx_tile_map)"), (rc, msg)


def test_check_refuses_reserved_words_and_bad_pointers(check):
    for i in range(4):
        q = good()
        q.reserved[i] = 1
        rc, msg = check(q)
        assert rc == ERR_ARG and "reserved" in msg
    q = good()
    film_bytes, record_bytes = 64 * 48 * 11 * 4, 2 * 3 * 40
    rc, msg = check(q, 0, 0x10000)
    assert rc == ERR_ARG and re.search(r"\bacc\b", msg)
    rc, msg = check(q, 0x10000, 0)
    assert rc == ERR_ARG and "records" in msg
    base = 0x1000000
    assert check(q, base, base + film_bytes) == (0, "") and check(q, base + record_bytes, base) == (0, "")  # back to back, either order
    for a, r in ((base, base), (base, base + film_bytes - 4), (base + record_bytes - 4, base), (base, base + 4)):
        for space in (0, 1):
            rc, msg = check(good(on_device=space), a, r)
            assert rc == ERR_ARG and "records" in msg, (a, r, msg)
        assert check(good(on_device=2), a, r) == (0, "")  # a device address and a host address are not compared


def test_the_limits_are_the_constants_of_check_and_kernel(check, host):
    hdr = open(os.path.join(CSRC, "tile_map_check.h")).read()
    lo, hi, xs = (int(re.search(rf"{n} = (\d+)", hdr).group(1)) for n in ("PHX_TILE_MAP_MIN_TILE", "PHX_TILE_MAP_MAX_TILE", "PHX_TILE_MAP_MAX_XSTRIDE"))
    assert (lo, hi, xs) == (4, 1024, 24)
    assert check(good(tile_width=lo, tile_height=hi))[0] == 0 and check(good(tile_width=lo - 1))[0] == check(good(tile_height=hi + 1))[0] == ERR_ARG
    kernel = open(os.path.join(CSRC, "tile_map.hip")).read()
    assert '#include "tile_map_check.h"' in kernel and "PHX_TILE_MAP_MAX_XSTRIDE" in kernel
    for extent, tile, want in ((1, 4, 1), (4, 4, 1), (5, 4, 2), (65536, 4, 16384), (65536, 1024, 64), (37, 8, 5), (29, 8, 4)):
        assert host.tm_tiles(extent, tile) == want


SANITIZER_WANT = {"good": None, "null-acc": "acc", "null-records": "records", "records-in-film": "records", "records-in-film-other-space": None,
                  "width": "width", "height": "height", "xstride-low": "xstride", "xstride-high": "xstride", "no-m2": "m2_offset", "m2-wrap": "m2_offset",
                  "no-samples": "samples_offset", "samples-in-m2": "samples_offset", "tile-width-low": "tile_width", "tile-width-high": "tile_width",
                  "tile-height-low": "tile_height", "tile-height-high": "tile_height", "on-device": "on_device", "tau-nan": "tau", "floor": "floor",
                  "reserved": "reserved"}


def test_the_check_under_the_sanitizers(tmp_path):
    """tile_map_host.cpp's own main() as a stand-alone program under AddressSanitizer and UBSan: its cases get the answers above, and the
    program ends without a report"""
    sources, flags = REGISTRY["tile_map_host"]
    exe = str(tmp_path / "tile_map_host_asan")
    subprocess.run([NL.CXX] + NL.SANITIZE + ["-DTILE_MAP_HOST_MAIN"] + NL.HOST_FLAGS + flags + ["-o", exe] + sources, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-2000:])
    got = {l.split()[0]: (int(l.split()[1]), l) for l in r.stdout.splitlines()}
    assert sorted(got) == sorted(SANITIZER_WANT)
    for name, field in SANITIZER_WANT.items():
        rc, line = got[name]
        assert (rc == 0) if field is None else (rc == ERR_ARG and re.search(rf"\b{field}\b", line)), line


# ---- 3. the model on hand-made films --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(37, 29), (65, 67)])
@pytest.mark.parametrize("ts", [8, 32, 64])
def test_the_grid_is_the_tile_queues_list(W, H, ts):
    """phx_tiles_make(W, H, ts, 0, 1), drained, against the model's grid and the package's"""
    from phosphorus_mk2_amd import xpu
    if not os.path.exists(xpu.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    q = xpu.Tiles.make(W, H, ts)
    made = [q.next() for _ in range(len(q))]
    assert q.next() is None
    assert made == tm.grid(W, H, ts, ts)
    g = xpu.tile_map_grid(W, H, ts)
    assert [(int(r["x"]), int(r["y"]), int(r["w"]), int(r["h"])) for r in g] == made
    film, _ = tm.synthetic_film((H, W))
    records, summary = tm.tile_map(film, 4, 7, ts, ts, 0.1, 0.0)
    assert [(int(r["x"]), int(r["y"]), int(r["w"]), int(r["h"])) for r in records] == made and summary["tiles"] == len(made)
    assert sum(int(r["w"]) * int(r["h"]) for r in records) == W * H == summary["pixels"]


def test_a_tile_list_queue_serves_its_list():
    """phx_tiles_make_list: the caller's tiles in the caller's order, a copy; count, reset and an empty list"""
    from phosphorus_mk2_amd import xpu
    if not os.path.exists(xpu.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    tiles = [(8, 0, 8, 8), (0, 0, 8, 8), (32, 24, 5, 5), (1000, 1000, 7, 3)]  # (no geometry is checked here: the frame's check is the only one)
    q = xpu.Tiles.from_list(tiles, 37, 29)
    assert len(q) == 4 and [q.next() for _ in range(4)] == tiles and q.next() is None and q.next() is None
    q.reset()
    assert q.next() == tiles[0] and len(q) == 4
    empty = xpu.Tiles.from_list([], 37, 29)
    assert len(empty) == 0 and empty.next() is None
    lib = xpu.load_library()
    assert not lib.phx_tiles_make_list(None, 3) and b"null list" in lib.phx_last_error()
    h = lib.phx_tiles_make_list(None, 0)
    assert h and lib.phx_tiles_count(h) == 0
    lib.phx_tiles_free(h)


@pytest.mark.parametrize("tau,floor", [(0.0, 0.0), (0.05, 0.01), (0.3, 0.0), (1e9, 1.0)])
def test_the_summary_is_accumulates(tau, floor):
    film, at = tm.synthetic_film((29, 37), 8, 4, 7)
    for ts in (8, (16, 4)):
        tw, th = (ts, ts) if isinstance(ts, int) else ts
        records, summary = tm.tile_map(film, 4, 7, tw, th, tau, floor)
        want = ac.summary(film, (0, 4, 7), tau, floor)
        assert {k: summary[k] for k in want} == want
        assert summary["open"] == sum(tm.is_open(r) for r in records) and summary["tiles"] == len(records)
    if tau == 1e9:
        # every valid pixel but "huge r" (L = 1e30 q against b b = 1e18) converges; what stays open holds that pixel or a starved one
        assert summary["converged"] == summary["pixels"] - summary["invalid"] - 1
        y, x = at["huge r"]
        assert summary["open"] == sum(int(r["starved"]) > 0 or (r["x"] <= x < r["x"] + r["w"] and r["y"] <= y < r["y"] + r["h"]) for r in records) > 0
    if tau == 0.3:
        assert 0 < summary["open"] <= summary["tiles"] and summary["converged"] > 0


def test_the_records_are_a_plain_loop_over_the_pixels():
    """the rule once more, pixel by pixel with Python floats (binary64) and math.sqrt, against the vectorised model"""
    film, _ = tm.synthetic_film((29, 37), 11, 7, 3, seed=3)
    tau, floor = float(F(0.2)), float(F(0.001))
    records, _ = tm.tile_map(film, 7, 3, 16, 4, tau, floor)
    for rec in records:
        invalid = starved = converged = samples = 0
        worst = F(0.0)
        for y in range(int(rec["y"]), int(rec["y"] + rec["h"])):
            for x in range(int(rec["x"]), int(rec["x"] + rec["w"])):
                px = film[y, x].astype(D).tolist()
                V, m, n = px[0:3], px[7:10], px[3]
                if not (all(math.isfinite(v) for v in V + m + [n]) and all(v >= 0 for v in m) and n >= 2):
                    invalid += 1
                    starved += int(math.isfinite(n) and 0 <= n < 2)
                    continue
                q = n / (n - 1.0)
                ok, r = True, 0.0
                for c in range(3):
                    L = m[c] * q
                    den = abs(V[c]) + floor
                    b = tau * den
                    ok = ok and L <= b * b
                    r = max(r, math.sqrt(L) / den if den > 0 else (0.0 if L == 0 else math.inf))
                converged += int(ok)
                samples += int(min(n, 2.0 ** 53))
                with np.errstate(over="ignore"):
                    worst = max(worst, F(r))
        assert (int(rec["invalid"]), int(rec["starved"]), int(rec["converged"]), int(rec["samples"])) == (invalid, starved, converged, samples)
        assert F(rec["worst"]).tobytes() == F(worst).tobytes()


def one_pixel_film(V=(1.0, 1.0, 1.0), m2=(0.01, 0.01, 0.01), n=8.0):
    """a 4 x 4 film (one tile) of ordinary converged pixels with pixel (1, 2) set to the arguments"""
    f = np.zeros((4, 4, 7), F)
    f[..., 0:3] = 1.0; f[..., 3:6] = 1e-6; f[..., 6] = 16.0
    f[1, 2, 0:3] = V; f[1, 2, 3:6] = m2; f[1, 2, 6] = n
    return f


def one(film, tau=0.1, floor=0.0):
    records, summary = tm.tile_map(film, 3, 6, 4, 4, tau, floor)
    assert len(records) == 1
    return records[0], summary


def test_each_special_pixel_lands_in_the_counter_the_rule_names():
    base, _ = one(one_pixel_film((1.0, 1.0, 1.0), (1e-6,) * 3, 16.0))
    assert (int(base["invalid"]), int(base["starved"]), int(base["converged"]), int(base["samples"])) == (0, 0, 16, 256) and not tm.is_open(base)
    # a NaN colour, an infinite m2, m2 < 0: invalid, not starved; the tile is not open for them: more samples never cure them
    for film in (one_pixel_film(V=(1.0, np.nan, 1.0)), one_pixel_film(m2=(0.01, np.inf, 0.01)), one_pixel_film(m2=(-1e-9, 0.0, 0.0)), one_pixel_film(n=np.nan),
                 one_pixel_film(n=-1.0), one_pixel_film(n=np.inf)):
        r, s = one(film)
        assert (int(r["invalid"]), int(r["starved"]), int(r["converged"]), int(r["samples"])) == (1, 0, 15, 240) and not tm.is_open(r) and s["open"] == 0
    # n = 0 and n = 1 (and 1.5): starved, which is also invalid, and the tile is open, whatever the other floats hold
    for film in (one_pixel_film(n=0.0), one_pixel_film(n=1.0), one_pixel_film(n=1.5), one_pixel_film(V=(np.nan,) * 3, m2=(-1.0,) * 3, n=0.0)):
        r, s = one(film)
        assert (int(r["invalid"]), int(r["starved"]), int(r["converged"]), int(r["samples"])) == (1, 1, 15, 240) and tm.is_open(r) and s["open"] == 1
    # n = 2 is valid: q = 2
    r, _ = one(one_pixel_film(m2=(0.004,) * 3, n=2.0))
    assert (int(r["invalid"]), int(r["converged"]), int(r["samples"])) == (0, 16, 242) and F(r["worst"]) == F(math.sqrt(float(F(0.004)) * 2.0))
    # n = 2^60: valid, counted as 2^53 samples; q = 1 to the last bit
    r, _ = one(one_pixel_film(n=2.0 ** 60))
    assert (int(r["invalid"]), int(r["samples"])) == (0, 240 + 2 ** 53) and F(r["worst"]) == F(math.sqrt(float(F(0.01))))
    # a valid pixel that misses the criterion opens the tile
    r, s = one(one_pixel_film(m2=(0.5, 0.0, 0.0)))
    assert (int(r["invalid"]), int(r["converged"])) == (0, 15) and tm.is_open(r) and s["open"] == 1


def test_worst_is_the_rules():
    q = 8.0 / 7.0
    # den == 0 with L == 0: r = 0, and the pixel is converged at any tau, tau = 0 included
    r, _ = one(one_pixel_film(V=(0.0,) * 3, m2=(0.0,) * 3), tau=0.0)
    assert int(r["converged"]) == 1 and F(r["worst"]) == F(math.sqrt(float(F(1e-6)) * (16.0 / 15.0)))  # (the other pixels' r)
    film = np.zeros((4, 4, 7), F); film[..., 6] = 8.0  # every pixel black with m2 == 0
    r, s = one(film, tau=0.0)
    assert (int(r["invalid"]), int(r["converged"])) == (0, 16) and r["worst"].tobytes() == F(0.0).tobytes() and not tm.is_open(r)
    # den == 0 with L > 0: r = +inf, never converged while floor == 0; a floor makes den > 0 and r finite
    film[1, 2, 3] = 0.25
    r, _ = one(film, tau=1e9)
    assert int(r["converged"]) == 15 and np.isposinf(r["worst"]) and tm.is_open(r)
    r, _ = one(film, tau=1e9, floor=0.5)
    assert int(r["converged"]) == 16 and F(r["worst"]) == F(math.sqrt(0.25 * q) / 0.5)
    # tau = 0: only m2 == 0 converges, and worst is what it is at any tau
    a, _ = one(one_pixel_film(), tau=0.0)
    b, _ = one(one_pixel_film(), tau=0.5)
    assert int(a["converged"]) == 0 and int(b["converged"]) == 16 and a["worst"].tobytes() == b["worst"].tobytes()
    assert F(a["worst"]) == F(math.sqrt(float(F(0.01)) * q) / 1.0)
    # the largest of the three colours, of the valid pixels only
    r, _ = one(one_pixel_film(V=(1.0, 2.0, 4.0), m2=(0.01, 0.09, 0.04)))
    assert F(r["worst"]) == F(max(math.sqrt(float(F(m)) * q) / v for m, v in ((0.01, 1.0), (0.09, 2.0), (0.04, 4.0))))
    r, _ = one(one_pixel_film(V=(1.0, np.nan, 1.0), m2=(1e6,) * 3))
    assert F(r["worst"]) == F(math.sqrt(float(F(1e-6)) * 16.0 / 15.0))  # the invalid pixel's m2 does not count
    # finite in binary64, +inf in fp32
    r, _ = one(one_pixel_film(V=(1e-30,) * 3, m2=(1e30,) * 3))
    assert np.isposinf(r["worst"]) and int(r["invalid"]) == 0
    # an all-invalid tile: worst == +0.0, and it is not open unless a pixel is starved
    film = one_pixel_film(); film[..., 0] = np.nan
    r, s = one(film)
    assert (int(r["invalid"]), int(r["starved"]), int(r["converged"]), int(r["samples"])) == (16, 0, 0, 0)
    assert r["worst"].tobytes() == F(0.0).tobytes() and not tm.is_open(r) and s["open"] == 0
    film[3, 3, 6] = 1.0
    r, s = one(film)
    assert (int(r["invalid"]), int(r["starved"])) == (16, 1) and r["worst"].tobytes() == F(0.0).tobytes() and tm.is_open(r) and s["open"] == 1


def test_the_synthetic_film_reaches_every_branch():
    film, at = tm.synthetic_film((29, 37), 8, 4, 7)
    assert sorted(at) == sorted(tm.SPECIALS)
    valid, starved, converged, r, n = tm.pixels(film, 4, 7, 0.1, 0.0)
    assert (~valid).sum() == 7 and starved.sum() == 2 and 0 < converged.sum() < valid.sum()
    assert not valid[at["NaN colour"]] and not valid[at["m2 < 0"]] and starved[at["n == 0"]] and starved[at["n == 1"]] and valid[at["n == 2"]] and valid[at["n == 2^60"]]
    assert r[at["den == 0, L == 0"]] == 0 and converged[at["den == 0, L == 0"]] and np.isposinf(r[at["den == 0, L > 0"]]) and np.isposinf(r[at["huge r"]])
    assert converged[at["m2 == 0"]] and np.isnan(film[..., 3]).any()  # and a foreign NaN nobody reads
    small, none = tm.synthetic_film((1, 9))
    assert not none and tm.pixels(small, 4, 7, 0.1, 0.0)[0].all()


def test_coverage_closes_a_tile_early():
    film = one_pixel_film(m2=(0.5, 0.0, 0.0))  # 15 of 16 converged
    r, _ = one(film)
    assert tm.is_open(r) and tm.is_open(r, 0.95) and not tm.is_open(r, 15 / 16) and not tm.is_open(r, 0.9)
    film[0, 0, 6] = 1.0  # a starved pixel keeps it open at any coverage
    r, _ = one(film)
    assert tm.is_open(r, 0.5)
    from phosphorus_mk2_amd import xpu
    records, _ = tm.tile_map(tm.synthetic_film((29, 37))[0], 4, 7, 8, 8, 0.3, 0.0)
    for cov in (1.0, 0.9, 0.5):
        assert xpu.open_tiles(records, cov) == tm.open_tiles(records, cov)


# ---- 4. the loop's pooling --------------------------------------------------------------------------------------------------------------------
def test_pooling_a_partial_frame_keeps_the_untouched_pixels_bits():
    """frame films with samples == 0 outside a subset of tiles: the accumulator's pixels there keep their bits (NaNs and foreign floats included),
    and the pixels inside pool as ever"""
    acc, frame, offs_a, offs_b = ac.synthetic_films((29, 37), 4, True, True)
    tiles = tm.grid(37, 29, 8, 8)
    subset = [tiles[k] for k in (1, 7, 19)]
    inside = np.zeros((29, 37), bool)
    for x, y, w, h in subset:
        inside[y:y + h, x:x + w] = True
    partial = np.where(inside[..., None], frame, F(0.0))
    assert not partial[~inside].any()
    out = ac.accumulate(acc, partial, offs_a, offs_b)
    full = ac.accumulate(acc, frame, offs_a, offs_b)
    n_a = acc[..., offs_a[2]]
    with np.errstate(invalid="ignore"):
        good_count = np.isfinite(n_a) & (n_a >= 0)  # (an accumulator pixel whose own count is NaN, infinite or negative is made NaN first, whatever n_b)
    keep = ~inside & good_count
    assert acc[keep].tobytes() == out[keep].tobytes() and keep.sum() > 800 and not np.isfinite(acc[keep]).all()
    assert ac.same(out[inside], full[inside]) and not ac.same(out[inside], acc[inside])


# The loop's recorded case.  Cornell 37 x 29 of frame_cases, 8 spp, depth 4, seeds 1, 2, 3; tile size 8: 5 x 4 = 20 tiles.  (TAU, FLOOR) was
# chosen here on the CPU with the oracle so that after two pooled frames the number of open tiles lies strictly between 0 and 20; the device
# is bit-identical to the oracle on this scene (tests/test_gpu_accumulate.py), so tests/test_gpu_tile_map.py reads the pair from here.
LOOP_W, LOOP_H, LOOP_TILE, LOOP_SPP, LOOP_DEPTH = 37, 29, 8, 8, 4
LOOP_TAU, LOOP_FLOOR = 0.5, 0.01
LOOP_OPEN_AFTER_TWO = 6             # of 20; after one frame 14 are open, so the loop's frames render 20, 14 and 6 tiles
LOOP_TILES_PER_FRAME = [20, 14, 6]
OFFS_ACC, OFFS_FRAME = (0, 4, 7), (0, 4, 0)


@functools.lru_cache(maxsize=None)
def _oracle_films(orc):
    from test_accumulate import moments_of
    scene = FC.SCENES["cornell"](LOOP_W, LOOP_H)

    def oracle_film(seed):
        """the oracle's frame of LOOP_SPP samples as a film with the m2 channel (H, W, 7): primary rgba, m2.  The oracle renders windows 8
        columns wide, so an odd width is covered strip by strip (frame_cases.strip_tiles), sample by sample"""
        film = np.zeros((LOOP_H, LOOP_W, 7), F)
        orc.set_tie_rule(True)
        try:
            O = orc.Oracle(scene, spp=LOOP_SPP, pps=1, depth=LOOP_DEPTH)
            for x, y, w, h in FC.strip_tiles(LOOP_W, LOOP_H):
                kw = dict(rng=orc.RNG_COUNTER, seed=seed, threads=1, tiles=[(x, y, w, h)])
                ys = np.stack([O.render(sample_begin=s, sample_end=s + 1, **kw)[0][:, x:x + w, :3] for s in range(LOOP_SPP)], axis=2)
                whole = O.render(**kw)[0][:, x:x + w]
                f, m2 = moments_of(np.ascontiguousarray(ys))
                assert bits_equal(f, whole[..., :3])  # the per-sample films add up to the frame
                film[:, x:x + w, 0:4] = whole; film[:, x:x + w, 4:7] = m2
            O.close()
        finally:
            orc.set_tie_rule(False)
        return film
    films = [oracle_film(seed) for seed in (1, 2, 3)]
    for f in films:
        f.setflags(write=False)
    return films


def model_chain(frames, tau, floor, tile=LOOP_TILE, coverage=1.0, min_frames=1):
    """the progressive loop by the models: per frame k (the frame's tile list, the accumulator after it).  frames: full uniform frame films
    (H, W, 7); a frame over a tile list is the full frame inside the list's tiles with samples = spp, and zero outside"""
    H, W = frames[0].shape[:2]
    acc = np.zeros((H, W, 8), F)
    out = []
    for k, frame in enumerate(frames):
        if k < min_frames:
            tiles = tm.grid(W, H, tile, tile)
        else:
            tiles = tm.open_tiles(tm.tile_map(acc, 4, 7, tile, tile, tau, floor)[0], coverage)
            if not tiles:
                break
        film = np.zeros((H, W, 8), F)
        for x, y, w, h in tiles:
            film[y:y + h, x:x + w, 0:7] = frame[y:y + h, x:x + w]
            film[y:y + h, x:x + w, 7] = LOOP_SPP
        acc = ac.accumulate(acc, film, OFFS_ACC, OFFS_ACC)
        out.append((tiles, acc))
    return out


def test_the_recorded_pair_leaves_some_tiles_open_after_two_frames(orc):
    frames = _oracle_films(orc)
    chain = model_chain(frames, LOOP_TAU, LOOP_FLOOR)
    assert [len(tiles) for tiles, _ in chain] == LOOP_TILES_PER_FRAME  # min_frames = 1: frame 0 renders all, the map decides from frame 1 on
    records, summary = tm.tile_map(chain[1][1], 4, 7, LOOP_TILE, LOOP_TILE, LOOP_TAU, LOOP_FLOOR)
    print(f"open tiles after two pooled frames at tau {LOOP_TAU}, floor {LOOP_FLOOR}: {summary['open']} of {summary['tiles']}")
    assert summary["tiles"] == 20 and 0 < summary["open"] < 20 and summary["open"] == LOOP_OPEN_AFTER_TWO
    assert summary["invalid"] == 0 and {k: summary[k] for k in ("pixels", "invalid", "converged", "samples")} == ac.summary(chain[1][1], OFFS_ACC, LOOP_TAU, LOOP_FLOOR)
    # the third frame renders the open tiles only, and the closed tiles' pixels keep their bits
    assert len(chain) == 3 and chain[2][0] == tm.open_tiles(records) and len(chain[2][0]) == summary["open"]
    closed = np.ones((LOOP_H, LOOP_W), bool)
    for x, y, w, h in chain[2][0]:
        closed[y:y + h, x:x + w] = False
    before, after = chain[1][1], chain[2][1]
    assert before[closed].tobytes() == after[closed].tobytes() and set(after[closed][:, 7].tolist()) == {8.0, 16.0} and (after[~closed][:, 7] == 24).all()
    assert not bits_equal(before[~closed], after[~closed])
