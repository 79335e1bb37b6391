"""The C++ adapter's sealed-block surface (include/dlsm_bloom_adapter.hpp):
FullFilterBlockBuilder::FinishBlock, host::ReadFilterBlock and
FullFilterBlockReader::FromBlock, compiled as a reference-side caller would
(-fno-rtti -fno-exceptions, no HIP headers) and checked against the oracle
(tests/cpp/adapter_block_test.cc)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compile(tmp_path):
    exe = tmp_path / "adapter_block_test"
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-fno-rtti", "-fno-exceptions", "-pthread",
           "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "adapter_block_test.cc"),
           "-L", os.path.join(ROOT, "dlsm_amd", "lib"), "-ldlsm_bloom",
           "-L", os.path.join(ROOT, "oracle"), "-loracle",
           "-Wl,-rpath," + os.path.join(ROOT, "dlsm_amd", "lib"),
           "-Wl,-rpath," + os.path.join(ROOT, "oracle"),
           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", str(exe)]
    subprocess.run(cmd, check=True)
    return exe


def test_finish_block_and_read_filter_block_on_cpu(tmp_path):
    """Builders with no context: the host loop builds the filter and seals it
    with dlsm_crc32c_extend / dlsm_crc32c_mask (the oracle's sealed bytes); a
    slot too small by 1..5 bytes gets the sealed match-everything filter (or
    nothing below 74 bytes) with DLSM_E_CAPACITY; host::ReadFilterBlock answers
    SHORT, CHECKSUM, TYPE in the reference's order (table/format.cc:389-441);
    FromBlock gives the reader of the block's contents.  Runs without a GPU."""
    exe = _compile(tmp_path)
    out = subprocess.run([str(exe), "cpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "OK adapter block cpu" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_finish_block_on_gpu(tmp_path):
    """FinishBlock through the reference-signature builder, staged keys,
    hash_in_addkey and a batcher (DLSM_BATCH_SEALED), each the oracle's sealed
    block with no host fallback counted; FromBlock + KeysMayMatch on the GPU
    equal the oracle's answers."""
    exe = _compile(tmp_path)
    out = subprocess.run([str(exe), "gpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "OK adapter block gpu" in out.stdout, out.stdout + out.stderr
