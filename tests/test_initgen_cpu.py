"""The seeding table (csrc/hz_initgen.hpp), padded and aligned for the seeding
loops' read-ahead, compiled on the host: entries 0-623 are
init_genrand(19650218)'s (_randommodule.c), the padding repeats the last, and
row 1 lies on a 64-byte boundary."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def init_genrand(s, n=624):
    mt = [s & 0xFFFFFFFF]
    for i in range(1, n):
        mt.append((1812433253 * (mt[-1] ^ (mt[-1] >> 30)) + i) & 0xFFFFFFFF)
    return mt


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_padded_table_is_init_genrand(tmp_path):
    exe = str(tmp_path / "initgen_driver")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe,
                        os.path.join(HERE, "initgen_driver.cpp")], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.split("\n")
    off, align, rows, pad = (int(x) for x in lines[0].split())
    words = [int(x) for x in lines[1:] if x]
    assert rows == 624 and pad >= 16 and len(words) == rows + pad
    want = init_genrand(19650218)
    assert words[:624] == want
    assert words[624:] == [want[-1]] * pad
    # rows 1, 9, 17, ...: the groups of eight the seeding loops load
    assert align == 64 and (off + 4) % 64 == 0
