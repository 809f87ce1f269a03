"""csrc/dispatch.h, the value -> template-argument helpers of every launch function: tests/dispatch_check.cpp is compiled with the host compiler of the
checker build and prints the tag each helper hands to its body.  No GPU."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emu  # noqa: E402

EXPECTED = """\
by_dtype 0: float(0)
by_dtype 1: f16(1)
by_dtype 2: bf16(2)
by_bool 0: false
by_bool 1: true
by_int 1: 1 -> true
by_int 2: 2 -> true
by_int 3: 3 -> true
by_int 4: 4 -> true
by_int 5: 5 -> true
by_int 0: 0 -> true
by_int 6: -> false
by_int -1: -> false
by_int 7: -> false
"""


def test_every_helper_calls_its_body_once_with_the_tag_of_the_value(tmp_path):
    exe = str(tmp_path / "dispatch_check")
    subprocess.run([build_emu.CLANG, "-x", "c++", "-std=c++17", "-O1", "-I", build_emu.HERE, "-I", build_emu.CSRC,
                    os.path.join(ROOT, "tests", "dispatch_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout.decode()
    # one tag per line: the body ran exactly once with the value asked for; an unlisted integer: not at all, and by_int says so
    assert out == EXPECTED
