"""Where a CPU test gets its host library, its sanitizer program and the text of include/phx_xpu.h from.

A host library is tests/native/host_*.cpp plus the files of csrc/ it wraps, compiled for the CPU and loaded through ctypes.  REGISTRY states each
one once: its sources and the flags beyond HOST_FLAGS.  load(name) builds tests/native/build/lib<name>.so when it is missing, when the compile
command is not the recorded one, or when a file THE COMPILER reported as a dependency (g++ -MM over all the sources) is newer than the library
or gone; the command and that list lie beside the library in lib<name>.so.json, so a warm call stats files and starts no compiler.  No test
module keeps a header list of its own, and none builds another module's library by a rule of its own.

The one exception is the host_bvh8 fixture of conftest.py (libhost_bvh8.so, -DPHX_STUDY_KNOBS=1): a conftest.py is one of the files by which
every change is tested, and no change edits it.  It keeps its own hand-written list and builds into tests/native/.

run_sanitized compiles the same sources as a stand-alone program (their own main() behind a -D) under AddressSanitizer and UBSan and runs it."""
import ctypes as C
import functools
import json
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "phosphorus_mk2_amd", "csrc")
BUILD = os.path.join(NATIVE, "build")
ERR_ARG = 1  # PHX_ERR_ARG
CXX = "g++"
HOST_FLAGS = ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off"]
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-static-libasan", "-static-libubsan"]


def _rocm_include():
    return os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def _entry(host, *csrc, flags=()):
    return [os.path.join(NATIVE, host)] + [os.path.join(CSRC, c) for c in csrc], list(flags)


FLATTEN = ["-D__HIP_PLATFORM_AMD__", "-I", _rocm_include()]  # scene_flatten.h and kernels.h include <hip/hip_runtime.h>, here for g++
REGISTRY = {  # name -> (sources, flags beyond HOST_FLAGS)
    "host_accumulate": _entry("host_accumulate.cpp", "accumulate_check.cpp"),
    "host_denoise": _entry("host_denoise.cpp", "denoise_check.cpp"),
    "host_display": _entry("host_display.cpp", "display_check.cpp"),
    "host_guides": _entry("host_guides.cpp", "guides_check.cpp"),
    "host_reproject": _entry("host_reproject.cpp", "reproject_check.cpp"),
    "host_outlier_clamp": _entry("host_outlier_clamp.cpp", "outlier_clamp_check.cpp"),
    "host_film_checks": _entry("host_film_checks.cpp"),
    "host_frame_plan": _entry("host_frame_plan.cpp", "frame_plan.cpp"),
    "host_mt_accept": _entry("host_mt_accept.cpp", flags=["-march=haswell", "-mfma"]),
    "host_flatten": _entry("host_flatten.cpp", "scene_flatten.cpp", flags=FLATTEN),
    "host_flatten_power": _entry("host_flatten_power.cpp", "scene_flatten.cpp", flags=FLATTEN),
    "host_flatten_env": _entry("host_flatten_env.cpp", "scene_flatten.cpp", flags=FLATTEN),
}


# ---- the libraries ------------------------------------------------------------------------------------------------------------------------
def _dependencies(args):
    """-> every file g++ -MM names for the compile `args` (all its sources; system headers left out by -MM), as absolute paths"""
    out = subprocess.run([CXX, "-MM"] + args, check=True, capture_output=True, text=True).stdout.replace("\\\n", " ")
    return sorted({os.path.abspath(f) for rule in out.splitlines() if ":" in rule for f in rule.split(":", 1)[1].split()})


def _stale(so, record, args):
    try:
        built = os.path.getmtime(so)
        with open(record) as f:
            was = json.load(f)
        return was["command"] != args or any(os.path.getmtime(d) > built for d in was["deps"])
    except (OSError, ValueError, KeyError):  # no library, no record, or a recorded dependency is gone
        return True


def ensure(name, registry=REGISTRY, out_dir=BUILD):
    """-> the path of lib<name>.so in out_dir, built first if it is stale.  It is built under another name and moved into place, so a compile
    that fails raises CalledProcessError and leaves the previous library and its record alone."""
    sources, flags = registry[name]
    so = os.path.join(out_dir, f"lib{name}.so")
    record = so + ".json"
    args = ["-O2", "-fPIC", "-shared"] + HOST_FLAGS + flags + sources
    if _stale(so, record, args):
        os.makedirs(out_dir, exist_ok=True)
        deps, tmp = _dependencies(args), f"{so}.{os.getpid()}.tmp"
        try:
            subprocess.run([CXX] + args + ["-o", tmp], check=True)
            os.replace(tmp, so)
            with open(tmp, "w") as f:
                json.dump({"command": args, "deps": deps}, f, indent=1)
            os.replace(tmp, record)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
    return so


def load(name, registry=REGISTRY, out_dir=BUILD):
    return C.CDLL(ensure(name, registry, out_dir))


def recorded_dependencies(name, out_dir=BUILD):
    with open(os.path.join(out_dir, f"lib{name}.so.json")) as f:
        return json.load(f)["deps"]


def run_sanitized(tmp_path, name, define=None):
    """the sources of `name` as a stand-alone program under AddressSanitizer and UBSan, `define` selecting their main(): it must end with
    status 0 and nothing on stderr -> its stdout"""
    sources, flags = REGISTRY[name]
    exe = str(tmp_path / f"{name}_asan")
    subprocess.run([CXX] + SANITIZE + ([f"-D{define}"] if define else []) + HOST_FLAGS + flags + ["-o", exe] + sources, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


def checker(lib, fn, argtypes, extra=()):
    """int lib.fn(argtypes ..., char* err, uint32_t err_bytes, extra ...) as a callable (arguments ..., extra arguments ...) -> (status, message)"""
    f = getattr(lib, fn)
    f.argtypes, f.restype = list(argtypes) + [C.c_char_p, C.c_uint32] + list(extra), C.c_int

    def call(*args):
        err = C.create_string_buffer(256)
        rc = f(*args[:len(argtypes)], err, 256, *args[len(argtypes):])
        return rc, err.value.decode()
    return call


def case_ids(cases):
    """parametrize ids of a list of keyword dicts: "k=v,k=v", or "defaults" for the empty one"""
    return [",".join(f"{k}={v}" for k, v in kw.items()) or "defaults" for kw in cases]


# ---- the header's text --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def header():
    with open(os.path.join(ROOT, "include", "phx_xpu.h")) as f:
        return f.read()


def struct_body(name, strip_comments=True):
    """the text between the braces of `typedef struct name { ... } name;`"""
    body = re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", header(), re.S).group(1)
    return re.sub(r"/\*.*?\*/", "", body, flags=re.S) if strip_comments else body


def flat(text):
    """a comment's text without its stars and with single spaces: what a phrase list is searched in"""
    return " ".join(text.replace("*", " ").split())
