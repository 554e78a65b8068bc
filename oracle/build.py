"""oracle/build.py — builds the CPU oracle (TEST INFRASTRUCTURE; nothing under cuda-path-tracer-ss_amd/ refers to it).

  _build/liboracle.so        oracle.cpp against the shared math header csrc/ptmath.h, -ffp-contract=off -fno-fast-math:
                             the bit-exact checker of the parity tests, and bench.py's cpu_baseline ("port")
  _build/liboracle_libm.so   the same source with -DORACLE_LIBM_MATH: libm float functions and plain vector arithmetic
                             (oracle/libm_math.h) — shares no arithmetic with the product; tests/test_oracle_libm.py

  _ref/libref_probe.so       the REFERENCE'S OWN sources compiled for the CPU with the oracle's flags, driven by ref_probe.cpp
                             (build_ref; only where the reference directory exists: PTSS_REFERENCE_DIR, default
                             /root/reference). As CUDA the reference cannot be built here (nvcc, cuRAND, Thrust, glm, GLUT);
                             its hot-path functions are plain C++ behind __device__, so oracle/ref_shim/ supplies stand-ins
                             of this repository's own for those headers, and the one construct g++ cannot parse — the
                             kernel<<<grid, block>>>(args) launch — is rewritten to REF_LAUNCH(kernel, grid, block, args) in
                             a copy of CudaTracer.cu under _ref/. Nothing of _ref/ is committed. tests/test_reference_*.py
                             hold the oracle, the host mirror's scenes and camera against this library."""
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INC = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "cuda-path-tracer-ss_amd", "csrc")   # ptmath.h only: the arithmetic both sides pin
OUT = os.path.join(HERE, "_build")
BASE = ["-O2", "-std=c++17", "-fPIC", "-mfma", "-mavx2", "-Wall", "-Wno-unused-function", "-fopenmp", "-shared"]


def _newer(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


def _sources():
    hs = [os.path.join(d, f) for d in (INC, CSRC, HERE) if os.path.isdir(d) for f in os.listdir(d) if f.endswith(".h")]
    return [os.path.join(HERE, "oracle.cpp")] + hs


def _run(cmd):
    print("+", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def build_oracle(force=False):
    os.makedirs(OUT, exist_ok=True)
    out = os.path.join(OUT, "liboracle.so")
    if force or _newer(out, _sources()):
        _run(["g++"] + BASE + ["-ffp-contract=off", "-fno-fast-math", "-I", INC, "-I", CSRC, os.path.join(HERE, "oracle.cpp"), "-o", out])
    return out


def build_oracle_libm(force=False):
    os.makedirs(OUT, exist_ok=True)
    out = os.path.join(OUT, "liboracle_libm.so")
    if force or _newer(out, _sources()):
        _run(["g++"] + BASE + ["-DORACLE_LIBM_MATH", "-I", INC, "-I", HERE, os.path.join(HERE, "oracle.cpp"), "-o", out])
    return out


REF_OUT = os.path.join(HERE, "_ref")
REF_LIB = os.path.join(REF_OUT, "libref_probe.so")
REF_SHIM = os.path.join(HERE, "ref_shim")
# a kernel launch, however the brackets are spaced: name <<< grid, block >>> (args);
_LAUNCH = re.compile(r"(\w+)\s*<\s*<\s*<\s*([^;<>]*?)\s*>\s*>\s*>\s*\(([^;]*?)\)\s*;")
_LAUNCH_OPEN = re.compile(r"<\s*<\s*<")


def reference_dir():
    return os.environ.get("PTSS_REFERENCE_DIR", "/root/reference")


def rewrite_launches(text):
    """The one rule: name<<<grid, block>>>(args); -> REF_LAUNCH(name, grid, block, args);  Raises unless every <<< was rewritten."""
    out, n = _LAUNCH.subn(lambda m: "REF_LAUNCH(%s, %s, %s);" % (m.group(1), m.group(2), m.group(3)), text)
    opened = len(_LAUNCH_OPEN.findall(text))
    if n != opened or _LAUNCH_OPEN.search(out):
        raise RuntimeError(f"rewrote {n} kernel launches, the file has {opened}")
    return out, n


def _shim_sources():
    shim = [os.path.join(d, f) for d, _, fs in os.walk(REF_SHIM) for f in fs]
    return shim + [os.path.join(HERE, "ref_probe.cpp"), os.path.abspath(__file__)]


def build_ref(force=False):
    """oracle/_ref/libref_probe.so from the reference's sources, or None where there is no reference directory. Raises on failure."""
    src = os.path.join(reference_dir(), "CudaTracer")
    if not os.path.isdir(src):
        print(f"oracle/build.py: no reference at {reference_dir()}: oracle/_ref/ is not built", flush=True)
        return None
    ref_sources = [os.path.join(src, f) for f in os.listdir(src) if f.endswith((".cu", ".cpp", ".h"))]
    if not (force or _newer(REF_LIB, _shim_sources() + ref_sources)):
        return REF_LIB
    os.makedirs(REF_OUT, exist_ok=True)
    with open(os.path.join(src, "CudaTracer.cu"), encoding="latin-1") as f:
        text, n = rewrite_launches(f.read())
    with open(os.path.join(REF_OUT, "CudaTracer.cu"), "w", encoding="latin-1") as f:
        f.write(text)
    print(f"oracle/build.py: {n} kernel launches rewritten to REF_LAUNCH in oracle/_ref/CudaTracer.cu", flush=True)
    # the oracle's flags; -w: the reference's own warnings are not ours to fix. _ref/ comes before the reference so that
    # "CudaTracer.cu" is the rewritten copy; ref_shim/ before both so that every library header is the stand-in.
    _run(["g++", "-O2", "-std=c++17", "-fPIC", "-fopenmp", "-shared", "-w", "-ffp-contract=off", "-fno-fast-math",
          "-include", os.path.join(REF_SHIM, "msvc_rand.h"), "-I", REF_SHIM, "-I", REF_OUT, "-I", src,
          os.path.join(HERE, "ref_probe.cpp"), "-o", REF_LIB])
    return REF_LIB


def build_ref_loudly(force=False):
    """build_ref for the in-tree build: a failure is shouted into the log and swallowed (the product does not need the reference;
    tests/test_reference_*.py FAIL when the reference is there and the library is not)."""
    try:
        return build_ref(force)
    except Exception as e:   # noqa: BLE001
        bar = "!" * 100
        print(f"{bar}\n!!! oracle/build.py: BUILDING THE REFERENCE FOR THE CPU FAILED: {e!r}\n!!! oracle/_ref/libref_probe.so is missing or "
              f"stale; tests/test_reference_*.py will fail.\n{bar}", flush=True)
        try:
            if os.path.exists(REF_LIB):
                os.remove(REF_LIB)   # never leave a stale library for the tests to pass against
        except OSError:
            pass
        return None


def build_all(force=False):
    outs = [build_oracle(force), build_oracle_libm(force)]
    ref = build_ref_loudly(force)
    return outs + ([ref] if ref else [])


if __name__ == "__main__":
    build_all("--force" in sys.argv)
