"""The C-ABI library loads on a box without a GPU, exports every symbol include/phx_xpu.h declares, its
struct layouts match the ctypes mirror, and — with no device — every compute entry point fails loudly
(no CPU fallback).  No compute calls are made here."""
import ctypes as C
import os
import re
import sys

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from phosphorus_mk2_amd import xpu
    if not os.path.exists(xpu.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return xpu.load_library()


def test_exports_every_declared_symbol(lib):
    from phosphorus_mk2_amd import abi
    hdr = open(os.path.join(ROOT, "include", "phx_xpu.h")).read()
    declared = set(re.findall(r"\b(phx_[a-z_]+)\s*\(", hdr)) - {"phx_next_tile_fn", "phx_add_tile_fn"}
    assert declared == set(abi.EXPORTS), declared ^ set(abi.EXPORTS)
    raw = C.CDLL(os.path.join(ROOT, "phosphorus_mk2_amd", "libphx_hip.so"))
    for s in declared:
        assert hasattr(raw, s), s


def test_struct_layouts(lib):
    from phosphorus_mk2_amd import abi
    for i, t in enumerate([abi.Options, abi.Lobe, abi.Material, abi.FaceSet, abi.Mesh, abi.Camera, abi.Scene, abi.Tile, abi.Frame, abi.Stats]):
        assert C.sizeof(t) == lib.phx_abi_sizeof(i), t.__name__


def test_header_is_plain_c():
    """the boundary is a C ABI: the header must compile as C99 with no C++ / torch types"""
    import subprocess
    src = '#include "phx_xpu.h"\nint main(void){ phx_options o; (void)o; return (int)sizeof(phx_scene) == 0; }\n'
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                   input=src.encode(), check=True)


def test_tile_queue_matches_reference_layout(lib):
    """job::tiles_t::make (src/jobs/tiles.hpp:49-89): row-major 32x32 tiles with edge remainders; rank/world shard."""
    from phosphorus_mk2_amd import dist, xpu
    q = xpu.Tiles.make(1280, 720, 32)
    assert len(q) == 40 * 23
    tiles = []
    while True:
        t = q.next()
        if t is None:
            break
        tiles.append(t)
    assert tiles[0] == (0, 0, 32, 32) and tiles[39] == (1248, 0, 32, 32) and tiles[-1] == (1248, 704, 32, 16)
    assert tiles == dist.shard_tiles(1280, 720, 32, 0, 1)
    assert q.next() is None
    q.reset()
    assert q.next() == (0, 0, 32, 32)
    for world in (2, 3, 8):
        got = []
        for r in range(world):
            qr = xpu.Tiles.make(100, 70, 32, r, world)
            mine = []
            while (t := qr.next()) is not None:
                mine.append(t)
            assert mine == dist.shard_tiles(100, 70, 32, r, world)
            got += mine
        assert sorted(got) == sorted(dist.shard_tiles(100, 70, 32, 0, 1))  # a partition of the film
    with pytest.raises(xpu.DeviceError):
        xpu.Tiles.make(64, 64, 32, rank=2, world=2)


def test_tile_shard_is_balanced_and_not_striped(lib):
    """the multi-GPU shard: every rank gets its fair share of tiles and touches every tile column and row band of the
    baseline film (plain 'tile id mod world' gives vertical stripes at 40 tiles per row)"""
    from phosphorus_mk2_amd import dist
    for world in (2, 3, 4, 6, 8):
        counts = []
        for r in range(world):
            mine = dist.shard_tiles(1280, 720, 32, r, world)
            counts.append(len(mine))
            assert len({x for x, _, _, _ in mine}) == 40, (world, r)
            assert len({y for _, y, _, _ in mine}) == 23, (world, r)
        assert sum(counts) == 40 * 23 and max(counts) - min(counts) <= 23, (world, counts)


def test_no_silent_cpu_fallback(lib):
    """Without a visible MI355X the device cannot be made; nothing renders on the host instead."""
    from phosphorus_mk2_amd import xpu
    n = C.c_int(-1)
    o = xpu.Options().pack()
    rc = lib.phx_discover(C.byref(o), C.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip("a GPU is visible: covered by the -m gpu tests")
    assert n.value == 0 and rc != 0 and lib.phx_last_error()
    with pytest.raises(xpu.DeviceError):
        xpu.HipDevice.make(xpu.Options())
    o.host_only = 1
    assert lib.phx_discover(C.byref(o), C.byref(n)) == 0 and n.value == 0  # --no-gpu is not an error
    assert lib.phx_dev_preprocess(None, None) != 0 and lib.phx_dev_join(None) != 0


def test_render_makes_one_device_on_a_multi_gpu_box(monkeypatch):
    """On a box with several GPUs render() (and every single-device script) makes exactly ONE device, with device_ordinal -1 =
    the caller's current GPU; discover() is what makes one per GPU — or only the one asked for."""
    from phosphorus_mk2_amd import scenes, xpu

    class FakeLib:
        def phx_discover(self, opts, n):
            n._obj.value = 4
            return 0

        def phx_last_error(self):
            return b""

    made = []

    class Stop(Exception):
        pass

    def fake_make(options):
        made.append(options.device_ordinal)
        raise Stop()

    monkeypatch.setattr(sys.modules[xpu.load_library.__module__], "load_library", lambda: FakeLib())  # where discover() looks it up
    monkeypatch.setattr(xpu.HipDevice, "make", staticmethod(fake_make))
    with pytest.raises(Stop):
        xpu.render(scenes.cornell(32, 32), spp=1)
    assert made == [-1]
    made.clear()

    def record_make(options):
        made.append(options.device_ordinal)
        return object()

    monkeypatch.setattr(xpu.HipDevice, "make", staticmethod(record_make))
    assert len(xpu.HipDevice.discover(xpu.Options())) == 4 and made == [0, 1, 2, 3]
    made.clear()
    assert len(xpu.HipDevice.discover(xpu.Options(device_ordinal=2))) == 1 and made == [2]


PATCH = os.path.join(ROOT, "integration", "reference.patch")
PATCH_PREIMAGE = os.path.join(ROOT, "tests", "golden", "reference_patch_preimage.json")


def parse_patch(path):
    """unified diff -> {file: [(old start, old count, pre-image bytes)]}; the pre-image is the hunk's context and removed lines, each
    with its newline, as they must stand in the unpatched file.  A hunk body is read by its header's counts, as patch(1) does, and
    every line outside a hunk must be a header line: a body longer or shorter than its header fails here."""
    import re
    files, hunks, cur, old_left, new_left = {}, None, None, 0, 0
    for line in open(path, "rb").read().split(b"\n")[:-1]:
        if old_left or new_left:
            tag = line[:1]
            assert tag in (b" ", b"-", b"+"), line
            if tag != b"+":
                cur[2] += line[1:] + b"\n"; old_left -= 1
            if tag != b"-":
                new_left -= 1
            assert old_left >= 0 and new_left >= 0, line
        elif line.startswith(b"--- a/"):
            hunks = files.setdefault(line[6:].decode(), [])
        elif line.startswith(b"@@"):
            m = re.match(rb"@@ -(\d+)(?:,(\d+))? \+(\d+)(?:,(\d+))? @@", line)
            cur = [int(m[1]), int(m[2] or 1), b""]
            old_left, new_left = cur[1], int(m[4] or 1)
            hunks.append(cur)
        else:
            assert line.startswith((b"diff ", b"+++ b/")), line
    assert not (old_left or new_left), "the last hunk is cut short"
    return {f: [tuple(h) for h in hs] for f, hs in files.items()}


def test_reference_patch_applies(tmp_path):
    """integration/reference.patch (the maintainer's change list: xpu_t::discover, four mesh_t accessors, the CMake source list,
    parsed_options_t::host_only) still applies to the reference tree, exactly where its hunks say.  The reference does not ship with
    this repository: tests/golden/reference_patch_preimage.json holds, for every hunk, the SHA-256 of the lines the reference has at
    that place (tests/golden/make_reference_patch_preimage.py), and the patch's own pre-image must hash to it.  Then the patch is
    dry-run against a tree that holds those pre-images at those lines: it must apply without offset or fuzz."""
    import hashlib
    import json
    import shutil
    import subprocess
    want = json.load(open(PATCH_PREIMAGE))["files"]
    got = parse_patch(PATCH)
    assert sorted(got) == sorted(want) and len(got) == 5
    for f, hunks in got.items():
        assert [(s, n) for s, n, _ in hunks] == [(h["start"], h["count"]) for h in want[f]["hunks"]], f
        for (start, n, pre), h in zip(hunks, want[f]["hunks"]):
            assert hashlib.sha256(pre).hexdigest() == h["sha256"], f"{f}: hunk at line {start} does not match the reference"
    if not shutil.which("patch"):
        return
    for f, hunks in got.items():  # the reference's line count, its hunk lines where they lie, placeholders elsewhere
        lines = [b"placeholder %d\n" % (i + 1) for i in range(want[f]["lines"])]
        for start, n, pre in hunks:
            lines[start - 1:start - 1 + n] = [l + b"\n" for l in pre.split(b"\n")[:-1]]
        p = tmp_path / f
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(b"".join(lines))
    r = subprocess.run(["patch", "-p1", "--dry-run", "--batch", "-d", str(tmp_path), "-i", PATCH], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("checking file") == 5 and "offset" not in r.stdout and "fuzz" not in r.stdout, r.stdout


def test_shade_kernel_constants_match_the_header():
    """abi's SHADE_* constants are the header's PHX_SHADE_* enumerators, read from its text; the kernel count is families x passes, fits the
    64 bits of phx_stats::shade_kernels, and every bit has a name of its own"""
    from phosphorus_mk2_amd import abi
    hdr = open(os.path.join(ROOT, "include", "phx_xpu.h")).read()
    declared = {name: int(value) for name, value in re.findall(r"\bPHX_SHADE_([A-Z0-9_]+)\s*=\s*(\d+)", hdr)}
    mirrored = {k[len("SHADE_"):]: v for k, v in vars(abi).items() if k.startswith("SHADE_") and isinstance(v, int)}
    assert declared == mirrored and len(declared) == 14, sorted(set(declared.items()) ^ set(mirrored.items()))
    assert abi.SHADE_KERNELS == abi.SHADE_FAMILIES * abi.SHADE_PASSES == 36 <= 64
    assert abi.SHADE_FAMILY_GENERAL + (abi.SHADE_G_PERHIT | abi.SHADE_G_TEX | abi.SHADE_G_ENV) + 1 == abi.SHADE_FAMILY_MASK
    assert re.search(r"uint64_t\s+shade_kernels;[^\n]*\n\} phx_stats;", hdr)  # appended: no earlier field moves
    assert abi.Stats._fields_[-1][0] == "shade_kernels"
    names = [abi.shade_kernel_name(b) for b in range(abi.SHADE_KERNELS)]
    assert len(set(names)) == abi.SHADE_KERNELS
    assert names[abi.shade_kernel_bit(abi.SHADE_FAMILY_LAMBERT1, abi.SHADE_PASS_LATER)] == "k_shade<2, false, false>"
    assert names[abi.shade_kernel_bit(abi.SHADE_FAMILY_MASK_ENV, abi.SHADE_PASS_LENS)].startswith("k_shade_g<true, true, true, true, true, true>")
    assert names[abi.shade_kernel_bit(abi.SHADE_FAMILY_GENERAL + abi.SHADE_G_TEX, abi.SHADE_PASS_CAMERA)].startswith("k_shade_g<false, true, false, true, false, false>")
    for bad in (-1, abi.SHADE_KERNELS):
        with pytest.raises(ValueError):
            abi.shade_kernel_name(bad)
    assert abi.shade_kernel_names(0b101) == [names[0], names[2]]
