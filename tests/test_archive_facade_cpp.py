"""include/vrhip/BrickArchive.hpp through examples/archive_playback.cpp: the program compiles with plain g++ against
the library, fails loudly without a GPU, and on one saves two timesteps, opens the first, loads the second into the
same set and finds every decode equal to the built sets' own."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compile(tmp_path, name="archive_playback"):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / name)
    lib = os.path.join(ROOT, "volumerenderer_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Werror", "-pthread", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", name + ".cpp"), "-L" + lib, "-lvrhip",
                           "-Wl,-rpath," + lib, "-o", exe])
    return exe


def test_archive_example_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = _compile(tmp_path)
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the gpu test")
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode != 0                      # no CPU fallback
    assert "no usable HIP device" in (r.stderr + r.stdout)


@pytest.mark.gpu
def test_archive_example_plays_back(tmp_path):
    exe = _compile(tmp_path)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    for t in range(2):
        assert os.path.getsize(str(tmp_path / ("timestep%d.vrbs" % t))) % 16 == 0
