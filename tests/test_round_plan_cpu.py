"""The transform batcher's round planner (csrc/gpu/round_plan.h) on the CPU: tests/c/round_plan_check.cpp,
a stand-alone program, built with ASan + UBSan (runtimes linked statically, so nothing is preloaded) and
run once.  It checks every plan against a naive model -- membership, group order, order inside a group,
metadata contents, array placement -- for seeded random rounds and the extremes of a full round, both
modes, both zero-copy values, max_conns 1, 2, 3 and 64; that Create's meta_cap holds every round of up to
4 * max_conns buffers; that a capacity one byte short is refused with nothing written; and that 65 536
buffers of one connection plan in linear time.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_round_plan_against_model(tmp_path):
    exe = tmp_path / "round_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "brb_framework_amd", "csrc", "gpu"),
                    os.path.join(ROOT, "tests", "c", "round_plan_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
