"""tests/native_lib.py, where every CPU test gets its host library from: when load() builds and when it does not, on a throw-away library of
two sources in tmp_path, and what the compiler reports for the real registry against the header lists the test modules used to keep by hand."""
import ctypes as C
import glob
import os
import subprocess

import pytest

import native_lib as NL

A_CPP = """#include "mid.h"
#if __has_include("maybe.h")
#include "maybe.h"
#endif
extern "C" int value() { return VALUE; }
"""
B_CPP = """#include "other.h"
#ifndef EXTRA
#define EXTRA 0
#endif
extern "C" int other() { return OTHER + EXTRA; }
"""


class Toy:
    """a.cpp -> mid.h -> deep.h (VALUE) and, while it is there, maybe.h; b.cpp -> other.h (OTHER): the header only the FIRST source reaches, and only
    through another header, is deep.h"""
    def __init__(self, tmp_path):
        self.dir, self.out = str(tmp_path / "src"), str(tmp_path / "out")
        os.mkdir(self.dir)
        for name, text in (("a.cpp", A_CPP), ("b.cpp", B_CPP), ("mid.h", '#include "deep.h"\n'), ("deep.h", "#define VALUE 7\n"),
                           ("other.h", "#define OTHER 3\n"), ("maybe.h", "\n")):
            self.write(name, text)
        self.registry = {"toy": ([self.path("a.cpp"), self.path("b.cpp")], [])}
        self.so = os.path.join(self.out, "libtoy.so")

    def path(self, name):
        return os.path.join(self.dir, name)

    def write(self, name, text):
        """... with an mtime a second past the library's, if there is one: no test waits for the clock"""
        with open(self.path(name), "w") as f:
            f.write(text)
        if os.path.exists(getattr(self, "so", "")):
            later = os.stat(self.so).st_mtime_ns + 10 ** 9
            os.utime(self.path(name), ns=(later, later))

    def ensure(self, registry=None):
        return NL.ensure("toy", registry or self.registry, self.out)

    def stamp(self):
        return os.stat(self.so).st_mtime_ns

    def deps(self):
        return [os.path.basename(d) for d in NL.recorded_dependencies("toy", self.out)]


@pytest.fixture
def toy(tmp_path):
    return Toy(tmp_path)


def test_the_first_load_builds_and_the_second_starts_no_compiler(toy, monkeypatch):
    lib = NL.load("toy", toy.registry, toy.out)
    assert (lib.value(), lib.other()) == (7, 3) and lib._name == toy.so
    assert sorted(toy.deps()) == ["a.cpp", "b.cpp", "deep.h", "maybe.h", "mid.h", "other.h"]  # both sources' files, the first source itself among them
    built = toy.stamp()
    monkeypatch.setattr(NL, "CXX", toy.path("no-such-compiler"))
    assert toy.ensure() == toy.so and toy.stamp() == built
    toy.write("other.h", "#define OTHER 4\n")  # ... and that compiler name is what a stale library would have started
    with pytest.raises(FileNotFoundError):
        toy.ensure()


def test_a_header_only_the_first_source_reaches_through_another_rebuilds(toy):
    built = (toy.ensure(), toy.stamp())[1]
    toy.write("deep.h", "#define VALUE 8\n")
    toy.ensure()
    assert toy.stamp() != built and C.CDLL(toy.so).value() == 8


def test_a_changed_flag_rebuilds(toy):
    built = (toy.ensure(), toy.stamp())[1]
    toy.ensure({"toy": (toy.registry["toy"][0], ["-DEXTRA=2"])})
    assert toy.stamp() != built and C.CDLL(toy.so).other() == 5


def test_a_deleted_dependency_rebuilds(toy):
    built = (toy.ensure(), toy.stamp())[1]
    os.remove(toy.path("maybe.h"))
    toy.ensure()
    assert toy.stamp() != built and "maybe.h" not in toy.deps() and "deep.h" in toy.deps()


def test_a_compile_error_raises_and_leaves_the_previous_library(toy):
    built = (toy.ensure(), toy.stamp())[1]
    record = open(toy.so + ".json").read()
    toy.write("b.cpp", "this is not C++\n")
    with pytest.raises(subprocess.CalledProcessError):
        toy.ensure()
    assert toy.stamp() == built and open(toy.so + ".json").read() == record and sorted(os.listdir(toy.out)) == ["libtoy.so", "libtoy.so.json"]
    lib = C.CDLL(toy.so)
    assert (lib.value(), lib.other()) == (7, 3)
    toy.write("b.cpp", B_CPP)  # mended: the next call builds
    toy.ensure()
    assert toy.stamp() != built


# ---- the real registry ----------------------------------------------------------------------------------------------------------------------
def deps(name):
    """what the compiler reported for `name`, as paths below the repository's root (what lies outside it, ROCm's headers, left out)"""
    NL.ensure(name)
    return {os.path.relpath(d, NL.ROOT) for d in NL.recorded_dependencies(name) if d.startswith(NL.ROOT + os.sep)}


def csrc(*names):
    return {f"phosphorus_mk2_amd/csrc/{n}" for n in names}


def test_the_registry_is_the_host_sources():
    """every tests/native/host_*.cpp is some entry's first source, but host_bvh8.cpp, which conftest.py builds"""
    hosts = {os.path.basename(p)[:-4] for p in glob.glob(os.path.join(NL.NATIVE, "host_*.cpp"))}
    assert {os.path.basename(src[0])[:-4]: name for name, (src, _) in NL.REGISTRY.items()} == {h: h for h in hosts - {"host_bvh8"}}
    assert all(os.path.exists(s) for src, _ in NL.REGISTRY.values() for s in src)


def test_the_compiler_reports_the_headers_the_hand_lists_missed():
    for name in ("host_accumulate", "host_denoise", "host_guides"):
        assert csrc("film_checks.h") <= deps(name), name
    assert csrc("display_rule.h", "phx_math.h") <= deps("host_display")
    for name in ("host_flatten", "host_flatten_power", "host_flatten_env"):
        assert csrc("scene_flatten.h", "kernels.h", "bsdf.h", "bvh8.h", "phx_math.h") <= deps(name), name


XPU_H = {"include/phx_xpu.h"}
FLATTEN_H = csrc("scene_flatten.cpp", "scene_flatten.h", "kernels.h", "bsdf.h", "bvh8.h", "phx_math.h") | XPU_H
# the lists the test modules kept by hand before this module, the sources among them (test_film_checks' list of the three libraries it rebuilt included)
HAND_LISTS = {
    "host_accumulate": csrc("accumulate_check.cpp", "accumulate_check.h", "film_checks.h") | XPU_H,
    "host_denoise": csrc("denoise_check.cpp", "denoise_check.h", "film_checks.h") | XPU_H,
    "host_guides": csrc("guides_check.cpp", "guides_check.h") | XPU_H,
    "host_display": csrc("display_check.cpp", "display_check.h", "display_rule.h", "film_checks.h", "phx_math.h") | XPU_H,
    "host_reproject": csrc("reproject_check.cpp", "reproject_check.h", "film_checks.h") | XPU_H,
    "host_outlier_clamp": csrc("outlier_clamp_check.cpp", "outlier_clamp_check.h", "film_checks.h") | XPU_H,
    "host_frame_plan": csrc("frame_plan.cpp", "frame_plan.h") | XPU_H,
    "host_mt_accept": csrc("bvh8.h", "phx_math.h"),
    "host_flatten": FLATTEN_H,
    "host_flatten_power": FLATTEN_H | {"tests/native/host_flatten.cpp"},
    "host_flatten_env": FLATTEN_H | {"tests/native/host_flatten.cpp", "tests/native/host_flatten_power.cpp"},
}


@pytest.mark.parametrize("name", list(HAND_LISTS))
def test_every_hand_list_is_within_what_the_compiler_reports(name):
    assert HAND_LISTS[name] | {f"tests/native/{name}.cpp"} <= deps(name)
