"""CPU-only checks of the workspace layout the scalar-chain entry points share (eks_amd/csrc/eks_chain_plan.hpp:
chain_layout): the five size queries against their closed form, and the host simulators' stand-alone programs, which
carve buffers of exactly the reported size with the same function, under AddressSanitizer + UBSan."""
import ctypes
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 32      # kChainChunk


def align256(nbytes):
    return (nbytes + 255) // 256 * 256


def geometry(T):
    nc = (T + CHUNK - 1) // CHUNK
    gs = math.isqrt(nc - 1) + 1 if nc > 1 else 1      # ceil(sqrt(nc))
    assert (gs - 1) ** 2 < nc <= gs * gs
    return nc, (nc + gs - 1) // gs


def expected_bytes(T, N, draws=0, part=False):
    """9 chunk planes and 9 group planes of float32; the sampler adds gam, hG and per-draw beta, hB; em, innovations and
    smooth_tv one float64 plane of chunk partials.  Every plane is rounded up to 256 bytes on its own."""
    nc, ng = geometry(T)
    total = 9 * align256(nc * N * 4) + 9 * align256(ng * N * 4)
    if draws:
        total += align256(nc * N * 4) + align256(draws * nc * N * 4) + align256(ng * N * 4) + align256(draws * ng * N * 4)
    if part:
        total += align256(nc * N * 8)
    return total


@pytest.fixture(scope='module')
def lib():
    from eks_amd import _build, _lib
    _build.build()
    return _lib.load()


@pytest.mark.parametrize('N', [1, 3, 65, 193])
def test_workspace_queries_match_the_closed_form(lib, N):
    from eks_amd import _lib
    for T in (1, 32, 33, 129, 2049, 100000):
        d = _lib.EksDims(N, T, 1, 1, _lib.FLAG_DIAG_MODEL | _lib.FLAG_VS_DIAG)
        ref = ctypes.byref(d)
        assert lib.eks_smooth_increments_workspace_bytes(ref) == expected_bytes(T, N), (T, N)
        for query in (lib.eks_em_stats_workspace_bytes, lib.eks_innovations_workspace_bytes,
                      lib.eks_smooth_tv_workspace_bytes):
            assert query(ref) == expected_bytes(T, N, part=True), (T, N)
        for draws in (1, 3):
            assert lib.eks_sample_workspace_bytes(ref, draws) == expected_bytes(T, N, draws=draws), (T, N, draws)


@pytest.mark.parametrize('sim', ['em', 'increments', 'innov', 'sample', 'smooth_tv'])
def test_simulator_programs_are_clean_under_sanitizers(sim, tmp_path):
    """Each tests/host_sim/<sim>_sim.cpp has a main() behind <SIM>_SIM_MAIN that runs every pass at odd sizes on a byte
    buffer of exactly chain_layout's size: a plane handed out beyond what the layout counts is a heap overflow here."""
    if not shutil.which('g++'):
        pytest.skip('no g++ here')
    flags = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    if subprocess.run(['g++', *flags, str(probe), '-o', str(tmp_path / 'probe')], capture_output=True).returncode != 0:
        pytest.skip('no g++ with the sanitizer runtimes here')
    exe = str(tmp_path / f'{sim}_sim')
    subprocess.run(['g++', '-std=c++17', '-O1', '-g', *flags, '-fno-omit-frame-pointer', f'-D{sim.upper()}_SIM_MAIN',
                    '-I', os.path.join(ROOT, 'eks_amd', 'csrc'), os.path.join(ROOT, 'tests', 'host_sim', f'{sim}_sim.cpp'),
                    '-o', exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert f'{sim}_sim: ok' in r.stdout
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
