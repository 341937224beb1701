"""The running-mean window every output producer keeps (MeanWindow, ucla-roms_amd/csrc/k_sink.h), on the CPU:
tests/mean_window.cpp includes the header's host part under plain g++ and checks navg, coef = 1/n and
cm1 = 1 - 1/n exactly, the sink that follows from them, and written() with and without avg."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mean_window(tmp_path):
    exe = str(tmp_path / "mean_window")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "ucla-roms_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "mean_window.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
