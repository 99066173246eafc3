"""The per-lane byte I/O primitives of the device headers on the CPU: tests/c/lane_io_check.cpp, a
stand-alone program that runs brb_io::Src / Snk / SectorSnk / BlockSrc, lower4 / add_marker,
tail_word_a4 / word_any, the base64 pieces (b64_piece.h) and SegWalk::start one lane at a time against
byte loops and the oracle, every range in a heap block that is exactly its dword hull.  Built with
ROCm's clang++ (g++ rejects ext_vector_type member access) against tests/c/host_shim, plain and with
ASan + UBSan, and run as a subprocess; nothing is preloaded.

What the GPU suite cannot see is the read half of "touches no dword that holds none of the range's
bytes": an over-read is masked off before it reaches a result.  Here it is ASan's redzone -- but only
with -DBRB_GLOBAL= (empty): the accessors dereference address_space(1) pointers, which ASan does not
instrument.  The positive controls pin both facts, and the mutants show that the sweeps reach each
guard.  No GPU.  Not covered: BlockSrcW, the word funnel's LDS ring, the kernels' own loops."""
import glob
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_DIR = os.path.join(ROOT, "brb_framework_amd", "csrc", "gpu")
SHIM = os.path.join(ROOT, "tests", "c", "host_shim")
HARNESS = os.path.join(ROOT, "tests", "c", "lane_io_check.cpp")
ORACLE_DIR = os.path.join(ROOT, "oracle")

PLAIN = ["-O1", "-g", "-Wall", "-Wextra", "-Werror"]
SAN = PLAIN + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DBRB_GLOBAL="]
SAN_NO_SEAM = PLAIN + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _llvm_bin():
    """llvm/bin of the ROCm whose hipcc builds the library (brb_framework_amd/Makefile: ROCM, HIPCC)."""
    rocm = os.environ.get("ROCM") or os.environ.get("ROCM_PATH") or "/opt/rocm"
    cands = [os.path.join(rocm, "llvm", "bin")]
    hipcc = shutil.which("hipcc")
    if hipcc:
        cands.append(os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "llvm", "bin"))
    for d in cands:
        if os.path.exists(os.path.join(d, "clang++")):
            return d
    raise AssertionError("clang++ not found beside hipcc (looked in: %s); it builds tests/c/lane_io_check.cpp"
                         % ", ".join(cands))


def _build(out_dir, name, flags, gpu_dir=GPU_DIR, harness=HARNESS):
    """One program: the harness and the oracle, both with `flags`.  Returns the executable's path."""
    llvm = _llvm_bin()
    os.makedirs(str(out_dir), exist_ok=True)
    exe = os.path.join(str(out_dir), name)
    obj = exe + "_oracle.o"
    c_flags = [f for f in flags if f not in ("-DBRB_GLOBAL=", "-Werror")]     # the oracle: the reference, as it is
    subprocess.run([os.path.join(llvm, "clang"), "-std=gnu11"] + c_flags +
                   ["-c", os.path.join(ORACLE_DIR, "brb_oracle.c"), "-o", obj], check=True)
    subprocess.run([os.path.join(llvm, "clang++"), "-std=c++17"] + flags +
                   ["-I", SHIM, "-I", gpu_dir, "-I", ORACLE_DIR, harness, obj, "-lm", "-lpthread", "-o", exe],
                   check=True)
    return exe


def _run(exe, *args):
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    sym = os.path.join(_llvm_bin(), "llvm-symbolizer")
    if os.path.exists(sym):
        env["ASAN_SYMBOLIZER_PATH"] = sym
    return subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=600, env=env)


_san_built = []


def _san_exe(tmp_path):
    """The sanitized program of the real headers, built by the first test that needs it."""
    if not (_san_built and os.path.exists(_san_built[0])):
        _san_built[:] = [_build(tmp_path, "lane_io_san", SAN)]
    return _san_built[0]


def test_plain_build(tmp_path):
    out = _run(_build(tmp_path, "lane_io_plain", PLAIN))
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


def test_sanitized_build(tmp_path):
    out = _run(_san_exe(tmp_path))
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout + out.stderr)[-4000:]


@pytest.mark.parametrize("plant", ["--plant-load", "--plant-store"])
def test_instrumentation_is_live(tmp_path, plant):
    """The real ldg() / stg() on the dword just past an exact-fit block must be reported."""
    out = _run(_san_exe(tmp_path), plant)
    assert out.returncode != 0, out.stdout + out.stderr
    assert "heap-buffer-overflow" in out.stderr, out.stderr[-4000:]
    assert "brb_gpu_common.h" in out.stderr, out.stderr[-4000:]


def test_asan_is_blind_without_the_seam(tmp_path):
    """Why BRB_GLOBAL can be predefined: with address_space(1) in place ASan does not instrument the
    accessors, and the planted over-read runs clean.  If a later toolchain instruments address space 1
    this fails: delete it then, with a note."""
    out = _run(_build(tmp_path, "lane_io_noseam", SAN_NO_SEAM), "--plant-load")
    assert out.returncode == 0 and "planted load done" in out.stdout, out.stdout + out.stderr


# (header, exact text that occurs once, replacement): each is one wrong comparison in a guard.  The
# first, second, fifth and seventh leave every value correct; only the sanitizer sees them.
MUTANTS = [
    ("src_next", "byte_stream.h", "rem > 4 - o", "rem >= 4 - o"),
    ("blocksrc_load", "byte_stream.h", "base + i < ndw", "base + i <= ndw"),
    ("blocksrc_init_below", "byte_stream.h", "ndw && !below", "ndw"),
    ("snk_put_hi", "byte_stream.h", "o + n - 1 < 3 ? o + n - 1 : 3u", "3u"),
    ("load_piece", "b64_piece.h", "4u * k < s + m", "4u * k <= s + m"),
    ("store_piece", "b64_piece.h", "first >= s + q", "first > s + q"),
    ("tail_word_a4", "brb_gpu_common.h", "o < t", "o <= t"),
]


@pytest.mark.parametrize("name,header,old,new", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_checks_bite(tmp_path, name, header, old, new):
    hdrs = tmp_path / "gpu"
    hdrs.mkdir()
    for h in glob.glob(os.path.join(GPU_DIR, "*.h")):
        shutil.copy(h, str(hdrs))
    harness = str(hdrs / "lane_io_check.cpp")     # beside the copies: its quoted includes find them first
    shutil.copy(HARNESS, harness)
    path = hdrs / header
    text = path.read_text()
    assert text.count(old) == 1, "%s: %r occurs %d times in %s" % (name, old, text.count(old), header)
    path.write_text(text.replace(old, new))
    # no -Werror: an edit may leave a variable unused, and the mutant must build to be judged by its run
    flags = [f for f in SAN if f != "-Werror"]
    out = _run(_build(tmp_path, "lane_io_" + name, flags, gpu_dir=str(hdrs), harness=harness))
    assert out.returncode != 0, "mutant %s survived:\n%s" % (name, (out.stdout + out.stderr)[-2000:])
