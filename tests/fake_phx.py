"""A recording stand-in for libphx_hip.so: every entry point of abi.EXPORTS answers PHX_OK (a make-like one a fresh handle) and appends
(name, arguments) to `calls`, so the host layer's loops run without a device and the order of their device calls can be read off
(tests/test_xpu_calls.py).  Nothing is rendered: films stay zero unless a script fills them.

    fake = fake_phx.install(monkeypatch, phx_dev_film_accumulate=lambda n, args: ...)

A script gets the 1-based count of its entry point's calls and the arguments as they were passed (a byref'd struct is args[i]._obj, an
address is an int): it may fill an output, and what it returns, unless None, is the call's status."""
import ctypes as C
import sys

import numpy as np

from phosphorus_mk2_amd import abi, xpu

MAKES = ("phx_dev_make", "phx_tiles_make", "phx_tiles_make_list")
UNORDERED = ("phx_tiles_free", "phx_last_error")  # the garbage collector places them


def _recorded(arg):
    """what is kept of one argument: a copy of a byref'd struct, the address of any other pointer, everything else as it is"""
    if hasattr(arg, "_obj"):
        return type(arg._obj).from_buffer_copy(arg._obj)
    if isinstance(arg, (C._Pointer, C.Array)):
        return C.cast(arg, C.c_void_p).value
    return arg


class FakePhx:
    def __init__(self, **script):
        self.calls, self.script, self.counts, self.handles = [], script, {}, 0
        self.tile_lists = []  # the tiles of every phx_tiles_make_list, copied while the caller's array is alive
        # HipDevice.start casts the library's own queue function to an address: a real function object, of a queue that is drained
        self.phx_tiles_next = abi.NEXT_TILE_FN(lambda user, out: self._call("phx_tiles_next", (user, C.cast(out, C.c_void_p).value)))

    def __getattr__(self, name):
        if name not in abi.EXPORTS:
            raise AttributeError(name)
        return lambda *args: self._call(name, args)

    def _call(self, name, args):
        n = self.counts[name] = self.counts.get(name, 0) + 1
        self.calls.append((name, tuple(_recorded(a) for a in args)))
        if name == "phx_tiles_make_list":
            self.tile_lists.append([(t.x, t.y, t.w, t.h) for t in args[0][:args[1]]])
        rc = self.script[name](n, args) if name in self.script else None
        if rc is not None:
            return rc
        if name in MAKES:
            self.handles += 1
            return 0x1000 * self.handles
        return b"" if name == "phx_last_error" else abi.PHX_OK

    # ---- reading the record ---------------------------------------------------------------------------------------------------------------
    def names(self):
        """the calls in order, without the prefix: "make", "start", "film_accumulate", "tiles_make" ..."""
        return [short(name) for name, _ in self.calls if name not in UNORDERED]

    def args(self, name):
        """the argument tuples of every call of `name` (short or full), in order"""
        return [a for n, a in self.calls if name in (n, short(n))]


def short(name):
    return name[len("phx_dev_"):] if name.startswith("phx_dev_") else name[len("phx_"):]


def install(monkeypatch, **script):
    """a fresh FakePhx in the place of the loader's cached library, for the test that asks"""
    fake = FakePhx(**script)
    monkeypatch.setattr(sys.modules[xpu.load_library.__module__], "_lib", fake)
    return fake


def plain(struct):
    """a struct's fields that are no addresses -> dict (nested structs as dicts, arrays as lists): what two traces can be compared by"""
    out = {}
    for field, ctype in struct._fields_:
        if ctype is C.c_void_p or issubclass(ctype, C._Pointer):
            continue
        v = getattr(struct, field)
        out[field] = plain(v) if isinstance(v, C.Structure) else list(v) if isinstance(v, C.Array) else v
    return out


def trace(fake):
    """the record without its addresses: per ordered call the name and the plain() of its structs; a tile queue's call keeps its numbers"""
    out = []
    for name, args in fake.calls:
        if name in UNORDERED:
            continue
        keep = args if name == "phx_tiles_make" else tuple(plain(a) for a in args if isinstance(a, C.Structure))
        out.append((name, keep))
    return out, fake.tile_lists


def fill_summary(args, index, **counts):
    """set fields of the summary struct a call got by reference at args[index]"""
    for k, v in counts.items():
        setattr(args[index]._obj, k, v)


def write_tile_records(args, converged):
    """fill the records of a phx_dev_film_tile_map call (args: dev, q, film, records, summary) with the grid of its q and, per tile,
    `converged` pixels (a sequence, one entry a tile)"""
    q = args[1]._obj
    grid = xpu.tile_map_grid(q.width, q.height, (q.tile_width, q.tile_height))
    grid["converged"] = converged
    records = np.frombuffer((C.c_char * grid.nbytes).from_address(args[3]), xpu.TILE_RECORD)
    records[:] = grid
