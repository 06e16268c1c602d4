"""The host halves of the class-activation-map entry points under AddressSanitizer + UndefinedBehaviorSanitizer: the build of
tests/test_host_sanitizers_ig.py (the library's sources `--offload-host-only -fsanitize=address,undefined`, the unchanged stand-in HIP
runtime tests/host_fuzz_stubs.cpp) with the stand-alone driver tests/host_fuzz_gradcam.hip, run as a program.  No GPU is involved."""
import concurrent.futures
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from test_host_sanitizers import CLANG, CSRC, HIPCC, NM, SAN, _digest

OUT = os.path.join(ROOT, "build", "host_san_gradcam")
DRIVER = os.path.join(ROOT, "tests", "host_fuzz_gradcam.hip")
STUBS = os.path.join(ROOT, "tests", "host_fuzz_stubs.cpp")
ITERS = 1500


def build_driver():
    """-> path of the sanitized driver (rebuilt when a source, a header or the driver changed)."""
    srcs = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))
    deps = srcs + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + [os.path.join(ROOT, "include", "stlt_hip.h"), DRIVER, STUBS]
    exe = os.path.join(OUT, f"host_fuzz_gradcam.{_digest(deps)}")
    if os.path.exists(exe):
        return exe
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    flags = ["--offload-host-only", *SAN, "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", CSRC]

    def cc(src):
        obj = os.path.join(OUT, os.path.splitext(os.path.basename(src))[0] + ".o")
        r = subprocess.run([HIPCC, *flags, "-c", src, "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        return obj

    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
        objs = list(ex.map(cc, srcs + [DRIVER]))
    # every host object references the fat binary its (absent) device pass would have embedded, under a per-file name
    und = subprocess.run([NM, "-u", *objs], capture_output=True, text=True, check=True).stdout
    names = sorted({ln.split()[-1] for ln in und.splitlines() if "__hip_fatbin_" in ln})
    fat = os.path.join(OUT, "fatbin_stubs.c")
    with open(fat, "w") as f:
        f.write("".join(f"char {n}[64];\n" for n in names))
    fat_o = os.path.join(OUT, "fatbin_stubs.o")
    subprocess.run([CLANG.replace("clang++", "clang"), "-c", fat, "-o", fat_o], check=True)
    stubs_o = os.path.join(OUT, "host_fuzz_stubs.o")
    subprocess.run([CLANG, *SAN, "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-c", STUBS, "-o", stubs_o], check=True)
    r = subprocess.run([HIPCC, "-fsanitize=address,undefined", "-fno-gpu-sanitize", *objs, fat_o, stubs_o, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
@pytest.mark.parametrize("seed", [1, 20261021])
def test_gradcam_launchers_are_clean_under_asan_and_ubsan(seed):
    exe = build_driver()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")  # the host side is what is under test, wherever this runs
    r = subprocess.run([exe, str(ITERS), str(seed)], capture_output=True, text=True, timeout=900, env=env)
    tail = (r.stdout[-1500:] + "\n" + r.stderr[-6000:])
    assert r.returncode == 0, tail
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, tail
    assert f"host_fuzz_gradcam: {ITERS} iterations" in r.stdout, tail
    # every entry point really walked its launch: none of the five is refused every time, and no launch it configured was impossible.
    # weights, map and upsample make two calls an iteration, one of them well-formed; the two trunk calls one, well-formed about half the time
    counts = r.stdout.split("calls that returned 0: ")[1].split("\n")[0].split()
    assert counts[0::2] == ["weights", "map", "upsample", "geometry", "backward_layer"], tail
    assert all(int(n) >= ITERS // 2 for n in counts[1:6:2]) and all(int(n) >= ITERS // 3 for n in counts[7::2]), tail
    assert int(r.stdout.split("kernel launches configured: ")[1].split()[0]) >= 5 * ITERS, tail
    assert int(r.stdout.split("refused by the runtime: ")[1].split()[0]) == 0, tail
