"""--gpuBAMcompression Host|Device: parsed by the host library, Device without a compressor installed fails before the first record is
written, and Host (the default) writes exactly what a run without the flag writes."""
import os
import struct

import pytest

from util import bam_parts, capi, oracle_lib, prepare, refstar, run_with_engine
import test_golden


def _argv(info, prefix, more):
    return ["--genomeDir", info["idx"], "--readFilesIn"] + info["fastq"] + ["--outFileNamePrefix", prefix] + more


@pytest.mark.parametrize("mode", ["Host", "Device"])
def test_flag_accepted(mode, tmp_path, built):
    run = capi.HostRun(_argv(test_golden._tiny_info(), str(tmp_path / "a_"), ["--outSAMtype", "BAM", "Unsorted", "--gpuBAMcompression", mode]))
    run.close()


@pytest.mark.parametrize("value", ["GPU", "device"])
def test_flag_rejected(value, tmp_path, built):
    with pytest.raises(RuntimeError, match="--gpuBAMcompression takes Host or Device"):
        capi.HostRun(_argv(test_golden._tiny_info(), str(tmp_path / "a_"), ["--outSAMtype", "BAM", "Unsorted", "--gpuBAMcompression", value]))


@pytest.mark.parametrize("types", [["Unsorted"], ["SortedByCoordinate"]])
def test_device_without_compressor_fails(types, tmp_path, built):
    info = dict(test_golden._tiny_info())
    info["extra"] = ["--outSAMtype", "BAM"] + types + ["--gpuBAMcompression", "Device"]
    with pytest.raises(RuntimeError, match="no device BGZF compressor is installed"):
        run_with_engine(info, str(tmp_path / "d_"), lambda g, p: oracle_lib.Oracle(g, p), batch_reads=300)


def _host_equals_default(info, tmp_path):
    d = str(tmp_path)
    outs = []
    for tag, more in (("plain", []), ("host", ["--gpuBAMcompression", "Host"])):
        i2 = dict(info)
        i2["extra"] = list(info.get("extra", [])) + ["--outSAMtype", "BAM", "Unsorted"] + more
        outs.append(run_with_engine(i2, os.path.join(d, tag + "_"), lambda g, p: oracle_lib.Oracle(g, p), batch_reads=700))
    a, b = record_members(outs[0] + "Aligned.out.bam"), record_members(outs[1] + "Aligned.out.bam")
    assert len(a) > 28 and a == b


def record_members(path):
    """the compressed bytes after the header block (which is compressed on its own and carries the command line in @PG / @CO)"""
    blob = open(path, "rb").read()
    text, refs, _ = bam_parts(path)
    need, p, got = 8 + len(text) + len(refs), 0, 0
    while got < need:
        bsize = struct.unpack("<H", blob[p + 16:p + 18])[0] + 1
        got += struct.unpack("<I", blob[p + bsize - 4:p + bsize])[0]
        p += bsize
    assert got == need
    return blob[p:]


def test_host_is_the_default_tiny(tmp_path, built):
    _host_equals_default(test_golden._tiny_info(), tmp_path)


@pytest.mark.skipif(not refstar.have_ref(), reason="oracle/_ref/STAR not built (no /root/reference here)")
def test_host_is_the_default_pe101(tmp_path, built):
    _host_equals_default(prepare("pe101", str(tmp_path), need_ref=False), tmp_path)
