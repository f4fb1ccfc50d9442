"""Compiling and running the tests' stand-alone host programs; holds no tests.  build_linked links a tests/cpp/*_host program
against libzang_hip.so; run_sanitized compiles a stand-alone program (its own main, nothing of it loaded into python) under
AddressSanitizer + UBSan, runs it and asserts its PASS; c_layout asks gcc for the sizes and offsets of include/zang_hip.h's
structs; flat_header is that header as one line of text; fnv1a is the checksum the host programs print."""
import ctypes
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "zang_hip.h")
SANITIZE = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
FNV_BASIS = 0xCBF29CE484222325


def build_linked(src, exe, extra=(), libs=()):
    """compile src (C++17, or C11 for a .c file) against include/ and link it with zang_amd/libzang_hip.so -> exe; `extra`:
    further compiler arguments before the source, `libs`: further libraries and linker arguments after libzang_hip"""
    import zang_amd  # noqa: F401  (fails loudly if libzang_hip.so is missing)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    lib = os.path.join(ROOT, "zang_amd")
    cc = ["gcc", "-std=c11", "-D_POSIX_C_SOURCE=200809L"] if src.endswith(".c") else ["g++", "-std=c++17"]
    subprocess.check_call(cc + ["-O1", "-Wall", "-Werror", "-I" + INCLUDE, *extra, src, "-L" + lib, "-lzang_hip", *libs, "-Wl,-rpath," + lib,
                                "-L" + rocm + "/lib", "-Wl,-rpath," + rocm + "/lib", "-o", exe])
    return exe


def build_sanitized(src, tmp_path, extra=()):
    """compile the stand-alone program src under AddressSanitizer + UBSan into tmp_path -> the executable's path"""
    exe = os.path.join(str(tmp_path), os.path.splitext(os.path.basename(src))[0])
    subprocess.check_call(SANITIZE + list(extra) + [src, "-o", exe])
    return exe


def run_sanitized(src, tmp_path, extra=()):
    """build_sanitized, then run it: exit 0, nothing on stderr, PASS as the last word -> its stdout"""
    r = subprocess.run([build_sanitized(src, tmp_path, extra)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr and r.stdout.strip().endswith("PASS"), r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def fnv1a(h, data):
    """64-bit FNV-1a of bytes `data`, continued from h (start: FNV_BASIS)"""
    for b in data:
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def flat_header():
    """include/zang_hip.h without comments, whitespace runs as one space"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return " ".join(text.split()).replace(" ,", ",")


def _c_lines(body):
    """the lines a C program with this main body prints, compiled against include/zang_hip.h"""
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "zang_hip.h"\nint main(void){' + body + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        with open(src, "w") as f:
            f.write(prog)
        subprocess.check_call(["gcc", "-I", INCLUDE, src, "-o", exe])
        return subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()


def c_layout(names):
    """names: {struct: [field, ...]} of include/zang_hip.h -> {struct: (sizeof, {field: offsetof})} as gcc lays them out"""
    body = ""
    for n, fields in names.items():
        body += f'printf("{n} - %zu\\n", sizeof({n}));'
        for f in fields:
            body += f'printf("{n} {f} %zu\\n", offsetof({n}, {f}));'
    out = {n: [None, {}] for n in names}
    for line in _c_lines(body):
        n, f, x = line.split()
        if f == "-":
            out[n][0] = int(x)
        else:
            out[n][1][f] = int(x)
    return {n: (size, offs) for n, (size, offs) in out.items()}


def c_ints(exprs):
    """the header's integer constant expressions, as gcc evaluates them -> [int]"""
    return [int(x) for x in _c_lines("".join(f'printf("%d\\n", (int)({e}));' for e in exprs))]


def mirror_layout(mirrors, offsets=True):
    """mirrors: {struct: its ctypes mirror}.  Asserts that gcc's sizeof -- and, with `offsets`, the offsetof of every field of
    the mirror -- is the mirror's -> (c_layout's result, the number of figures compared)"""
    lay = c_layout({n: [f for f, _ in t._fields_] if offsets else [] for n, t in mirrors.items()})
    seen = 0
    for n, (size, offs) in lay.items():
        assert size == ctypes.sizeof(mirrors[n]), (n, "-", ctypes.sizeof(mirrors[n]), size)
        for f, x in offs.items():
            assert getattr(mirrors[n], f).offset == x, (n, f, getattr(mirrors[n], f).offset, x)
        seen += 1 + len(offs)
    assert sorted(lay) == sorted(mirrors)
    return lay, seen
