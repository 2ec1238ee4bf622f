"""The checkpoint tensor-file reader (csrc/runtime/tensor_file.{h,cpp}) checked
on the CPU: tests/tensor_file_check.cpp is compiled with tensor_file.cpp for
the host, under the address and undefined-behaviour sanitizers, and run as a
child process on files written here with numpy.  fp16 and fp32 files read as
either type (round to nearest even one way, exact the other), the not-found /
wrong-size outcomes with guard words behind the buffer, and the K/V row
replication of GQA checkpoints."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RDIR = os.path.join(ROOT, "flexflow_amd", "csrc", "runtime")
HIPCC = "/opt/rocm/bin/hipcc"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _compilers(tmp):
    """g++ if it has _Float16 (x86-64: GCC 12 on), otherwise hipcc's host compiler;
    the sanitizer runtimes linked statically: no demand on the process's library order"""
    probe = os.path.join(tmp, "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { _Float16 h = (_Float16)1.5f; return (float)h == 1.5f ? 0 : 1; }\n")
    if shutil.which("g++") and subprocess.run(
            ["g++", "-std=c++17", probe, "-o", os.path.join(tmp, "probe")],
            capture_output=True).returncode == 0:
        return ["g++", "-std=c++17", "-O2", "-g", *SAN, "-static-libasan", "-static-libubsan"]
    if os.path.exists(HIPCC):
        return [HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g",
                "-I/opt/rocm/include", *SAN, "-static-libsan"]
    return None


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("tensor_file"))
    cc = _compilers(tmp)
    if cc is None:
        pytest.skip("no host compiler with _Float16")
    exe = os.path.join(tmp, "tensor_file_check")
    subprocess.run([*cc, os.path.join(ROOT, "tests", "tensor_file_check.cpp"),
                    os.path.join(RDIR, "tensor_file.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)

    def run(*args):
        p = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
        assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
        return p.stdout.strip()
    return run


def _read(check, tmp_path, mode, path, n):
    out = str(tmp_path / "out.bin")
    if os.path.exists(out):
        os.remove(out)
    outcome = check(mode, path, n, out)
    dt = np.uint16 if mode == "f16" else np.float32
    return outcome, (np.fromfile(out, dtype=dt) if outcome == "ok" else None)


def test_fp16_file_as_fp16_keeps_the_bits(check, tmp_path):
    n = 4099  # not a multiple of any buffer size
    bits = np.random.default_rng(1).integers(0, 1 << 16, n, dtype=np.uint16)
    path = str(tmp_path / "w16")
    bits.tofile(path)
    outcome, got = _read(check, tmp_path, "f16", path, n)
    assert outcome == "ok" and np.array_equal(got, bits)


def test_fp32_file_as_fp16_rounds_to_nearest_even(check, tmp_path):
    f32 = np.float32
    up = lambda x: np.nextafter(f32(x), f32(np.inf))
    down = lambda x: np.nextafter(f32(x), f32(-np.inf))
    special = [0.0, -0.0, 65504.0, -65504.0,
               down(65520.0), 65520.0, up(65520.0), -down(65520.0), -65520.0, -up(65520.0),
               2.0 ** -24, 2.0 ** -25, up(2.0 ** -25), down(2.0 ** -25), 3 * 2.0 ** -25,
               2.0 ** -14, down(2.0 ** -14), 2.0 ** -14 - 2.0 ** -25, 1e-10, -1e-10,
               1 + 2.0 ** -11, up(1 + 2.0 ** -11), down(1 + 2.0 ** -11), 1 + 3 * 2.0 ** -11,
               -(1 + 2.0 ** -11), 2048.0 + 1.0, 2048.0 + 3.0,
               np.inf, -np.inf, np.nan, 3.0e38, -3.0e38]
    rng = np.random.default_rng(2)
    bulk = (rng.standard_normal(4099) * np.exp2(rng.integers(-30, 18, 4099))).astype(np.float32)
    x = np.concatenate([np.array(special, dtype=np.float32), bulk])
    path = str(tmp_path / "w32")
    x.tofile(path)
    with np.errstate(over="ignore"):
        want = x.astype(np.float16)
    outcome, got = _read(check, tmp_path, "f16", path, x.size)
    assert outcome == "ok"
    nan = np.isnan(want)
    assert nan.sum() == 1 and np.array_equal(np.isnan(got.view(np.float16)), nan)
    assert np.array_equal(got[~nan], want.view(np.uint16)[~nan])


def test_fp16_file_as_fp32_widens_every_bit_pattern(check, tmp_path):
    bits = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    path = str(tmp_path / "all16")
    bits.tofile(path)
    want = bits.view(np.float16).astype(np.float32)
    outcome, got = _read(check, tmp_path, "f32", path, bits.size)
    assert outcome == "ok"
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def test_fp32_file_as_fp32_keeps_the_bits(check, tmp_path):
    bits = np.random.default_rng(3).integers(0, 1 << 32, 4099, dtype=np.uint32)
    path = str(tmp_path / "w32raw")
    bits.tofile(path)
    outcome, got = _read(check, tmp_path, "f32", path, bits.size)
    assert outcome == "ok" and np.array_equal(got.view(np.uint32), bits)


@pytest.mark.parametrize("mode,elem", [("f16", 2), ("f32", 4)])
def test_outcomes_and_guard_words(check, tmp_path, mode, elem):
    """(the check program fails if a read touched the words behind its n elements)"""
    n = 1000
    other = 6 - elem
    for width in (elem, other):
        for delta, want in ((0, "ok"), (-1, "wrong_size"), (1, "wrong_size")):
            path = str(tmp_path / f"f_{width}_{delta + 1}")
            with open(path, "wb") as f:
                f.write(bytes(n * width + delta))
            assert _read(check, tmp_path, mode, path, n)[0] == want, (width, delta)
    empty = str(tmp_path / "empty")
    open(empty, "wb").close()
    assert _read(check, tmp_path, mode, empty, n)[0] == "wrong_size"
    assert _read(check, tmp_path, mode, str(tmp_path / "missing"), n)[0] == "not_found"


@pytest.mark.parametrize("heads,kv_heads", [(8, 2), (4, 1)])
@pytest.mark.parametrize("mode,dt", [("rep16", np.uint16), ("rep32", np.float32)])
def test_kv_replication_is_repeat_over_the_head_axis(check, tmp_path, heads, kv_heads, mode, dt):
    d, H = 3, 5
    src = np.arange(kv_heads * d * H).astype(dt).reshape(kv_heads, d, H)
    inp, out = str(tmp_path / "kv_in"), str(tmp_path / "kv_out")
    src.tofile(inp)
    check(mode, heads, kv_heads, src.size, inp, out)
    want = np.repeat(src, heads // kv_heads, axis=0)
    assert np.array_equal(np.fromfile(out, dtype=dt).reshape(heads, d, H), want)
