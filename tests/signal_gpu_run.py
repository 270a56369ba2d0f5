"""Child process of tests/test_gpu_signal.py: one GPU step, under the time limit the parent sets.
    signal_gpu_run.py lib <workdir> <out.pkl>        test_signal_emul.vectors() through libstaramd.so: the tool mode with --gpuSignal Device (the host-records
                                                     entry) for every option combination, and the sorter's finish with the tracks
    signal_gpu_run.py many <bam> <prefix> <out.pkl>  the tool mode with --gpuSignal Device on a BAM file the parent wrote: more occupied tiles than
                                                     k_signal_tiles has workgroups"""
import os
import pickle
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from util import capi  # noqa: E402
import test_signal_emul as G  # noqa: E402


def cases(name):
    return [(opt, prefix) for prefix in (None, "chr") if not prefix or name in ("skips_refs", "mix") for opt in G.options(name)]


SORTER_OPTS = [("bg", 1, 1, 0), ("wig", 0, 0, 0), ("bg", 1, 0, 1), ("bg", 0, 1, 2)]


def lib_step(work, out_path):
    sg = capi.SignalDevice()
    sg.install()
    got = {"constants": (sg.tile, sg.chunk)}
    bz = capi.BgzfDevice(device=0)
    try:
        for name, recs in G.vectors().items():
            bam = G.write_bam(os.path.join(work, name + ".bam"), recs)
            for opt, prefix in cases(name):
                flags = G.wig_flags(*opt, prefix=prefix)
                got[("tool", name, opt, prefix)] = G.tool_mode(bam, os.path.join(work, "%s_d%s_" % (name, G.flag_tag(flags))), flags, device=True)
            n = len(recs)
            cuts = [c for c in (n // 3, n // 2) if 0 < c < n]
            for k, opt in enumerate(SORTER_OPTS):
                out, files = G.sorter_case(sg, bz, None, recs, cuts, opt, work, "%s_s%d" % (name, k), shuffle=random.Random(k) if k % 2 else None)
                got[("sorter", name, opt)] = (files, out)
    finally:
        bz.close()
        capi.SignalDevice.uninstall()
    pickle.dump(got, open(out_path, "wb"))


def many_step(bam, prefix, out_path):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sg = capi.SignalDevice()
    sg.install()
    try:
        files = G.tool_mode(bam, prefix, G.wig_flags("bg", 1, 1, 0) + ["--runThreadN", "3"], device=True)
    finally:
        capi.SignalDevice.uninstall()
    pickle.dump({"cus": cus, "files": files}, open(out_path, "wb"))


if __name__ == "__main__":
    {"lib": lib_step, "many": many_step}[sys.argv[1]](*sys.argv[2:])
