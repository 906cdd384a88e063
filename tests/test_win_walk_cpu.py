"""Schedule of the walk form of the windowed replay (eks_amd/csrc/eks_win_walk.hpp, the header eks_diag.hip's
replay_walk_block reads): tests/host_sim/win_walk_sim.cpp, a stand-alone program built with the address and
undefined-behaviour sanitizers, plays the waves, steps and LDS rings of a block for every number of chunks from 1 to 200
and every run length from 1 to 30 and checks that

  - every own chunk is replayed exactly once, by the wave that holds its rows;
  - every chunk is loaded once per run, plus at most four (the two halos at the run's ends);
  - every element and stand-in row a replay reads was written in this or the previous step and is not overwritten by the
    writes of the following step, which the single barrier per step lets overlap with the reads;
  - no wave loads a chunk while the rows of another are still live in its registers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_chunk_count_and_run_length(tmp_path):
    cxx = shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'win_walk_sim')
    subprocess.run([cxx, '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                    '-I', os.path.join(ROOT, 'eks_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'host_sim', 'win_walk_sim.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe, '200', '30'], capture_output=True, text=True)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith('ok 6000 cases')
