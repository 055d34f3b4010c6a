"""One way to build and run the stand-alone test programs (tests/*_prog.cpp, each with its own main) and to compare a C struct of the
public header with its ctypes class.  An ordinary module: the tests and the case modules import it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
PKG = os.path.join(ROOT, "sivo_amd")
INCLUDE = [os.path.join(PKG, "csrc"), os.path.join(PKG, "api"), os.path.join(PKG, "api", "orbslam"), TESTS]
BASE = ["g++", "-std=c++14", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off"]
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]

_built = {}          # (name, sanitize, link_lib, defines, include) -> executable, for this process
_probe = []          # [whether a trivial main links under SANITIZE], once it is known


def build(name, out_dir, *, sanitize=False, link_lib=False, defines=(), include=()):
    """tests/<name>.cpp compiled into out_dir; the executable's path.  link_lib: True for libsivo_hip, or the names of the package's
    libraries to link, in link order.  A second request with the same arguments (out_dir aside) gets the first one's executable while it
    exists."""
    libs = ("sivo_hip",) if link_lib is True else tuple(link_lib or ())
    key = (name, sanitize, libs, tuple(defines), tuple(include))
    if key in _built and os.path.exists(_built[key]):
        return _built[key]
    exe = os.path.join(str(out_dir), "_".join([name, *defines, *libs] + ["san"] * sanitize))
    cmd = BASE + (SANITIZE if sanitize else ["-O2"]) + ["-D" + d for d in defines] + ["-I" + d for d in (*INCLUDE, *include)]
    cmd += [os.path.join(TESTS, name + ".cpp"), "-o", exe]
    if libs:
        cmd += ["-L" + PKG, *("-l" + x for x in libs), "-Wl,-rpath," + PKG]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    _built[key] = exe
    return exe


def sanitizer_runtime_present(out_dir):
    """Whether g++ can compile and link a trivial main with the sanitizer flags: decided before any program under test is compiled, so a
    missing runtime (libasan / libubsan) reads as a skip and a finding in a program as a failure."""
    if not _probe:
        src, exe = os.path.join(str(out_dir), "san_probe.cpp"), os.path.join(str(out_dir), "san_probe")
        with open(src, "w") as f:
            f.write("int main() { return 0; }\n")
        _probe.append(subprocess.run([*BASE, *SANITIZE, src, "-o", exe], capture_output=True, text=True, timeout=120).returncode == 0)
    return _probe[0]


def run(exe, tmp_path, mode, blob, *, extra_args=(), timeout=300):
    """`exe mode [extra_args] <mode>.in <mode>.out` on the blob; the bytes it wrote."""
    fin, fout = tmp_path / (mode + ".in"), tmp_path / (mode + ".out")
    fin.write_bytes(blob)
    r = subprocess.run([exe, mode, *map(str, extra_args), str(fin), str(fout)], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (mode, r.returncode, r.stderr[-3000:])
    return fout.read_bytes()


def run_text(exe, args, text, timeout):
    """The programs that speak text: `exe args` with text on stdin; its stdout."""
    r = subprocess.run([exe, *map(str, args)], input=text, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return r.stdout


def c_layout(tmp_path, c_type, ctypes_cls, header="sivo_hip.h"):
    """sizeof and every offsetof of the header's c_type, as gcc lays it out, equal those of the ctypes class."""
    import ctypes
    fields = [f[0] for f in ctypes_cls._fields_]
    src, exe = tmp_path / (c_type + "_layout.c"), str(tmp_path / (c_type + "_layout"))
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{header}"\nint main(void) {{\n  printf("%zu", sizeof({c_type}));\n'
                   + "".join(f'  printf(" %zu", offsetof({c_type}, {f}));\n' for f in fields) + "  return 0;\n}\n")
    r = subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()]
    want = [ctypes.sizeof(ctypes_cls)] + [getattr(ctypes_cls, f).offset for f in fields]
    assert got == want, (c_type, got, want)
