"""The reader of pipeline 2's draw cuts with six draw stages (csrc/hz_host.hpp:
env_p2_dcuts, behind HZ_P2_DCUTS) under AddressSanitizer +
UndefinedBehaviorSanitizer, without a GPU: tests/host_dcuts6_driver.cpp has
its own main, runs as its own process with nothing preloaded, and checks
four-value and five-value settings, junk, and sets the gap rule rejects
against values written out in the driver."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_draw_cut_reader_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "host_dcuts6_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-o", exe,
           os.path.join(HERE, "host_dcuts6_driver.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith("HZ_")}
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "runtime error" not in p.stderr and "ERROR: AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    assert "host dcuts6 driver ok" in p.stdout, p.stdout[-2000:]
