"""Child process of tests/test_gpu_bgzf.py: one GPU step, under the time limit the parent sets.
    bgzf_gpu_run.py lib <vectors.pkl> <out.pkl>                   the vectors through libstaramd.so's compressor, one call each, then from 4 threads at once
    bgzf_gpu_run.py run <info.pkl> <prefix> Host|Device <batch>   alignReads with capi.Engine, BAM records compressed as the mode says
    bgzf_gpu_run.py many <out.pkl>                                test_bgzf_emul.many_calls: one call of more than 3 x as many blocks as workgroups"""
import os
import pickle
import sys
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from util import capi  # noqa: E402
import test_bgzf_emul as E  # noqa: E402


def lib_step(vec_path, out_path):
    vecs = pickle.load(open(vec_path, "rb"))
    bz = capi.BgzfDevice(device=0)
    single = {(lv, k): bz.compress(lv, segs) for lv in E.LEVELS for k, segs in vecs.items()}
    threads, errs = {}, []

    def work(i):
        try:
            for lv in E.LEVELS:
                for k, segs in vecs.items():
                    threads[(i, lv, k)] = bz.compress(lv, segs)
        except Exception as e:          # noqa: BLE001  (reported by the parent)
            errs.append(repr(e))
    th = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    bz.close()
    if errs:
        raise RuntimeError(errs[0])
    pickle.dump({"single": single, "threads": threads}, open(out_path, "wb"))


def run_step(info_path, prefix, mode, batch):
    info = pickle.load(open(info_path, "rb"))
    bz = capi.BgzfDevice(device=0) if mode == "Device" else None
    try:
        E.run_with_bgzf(info, prefix, lambda g, p: capi.Engine(g, p, device=0, max_reads=4096), bz, batch_reads=int(batch))
    finally:
        if bz is not None:
            bz.close()


def many_step(out_path):
    import torch
    grid = 2 * torch.cuda.get_device_properties(0).multi_processor_count         # staramd_bgzf_create: two workgroups per CU
    bz = capi.BgzfDevice(device=0)
    try:
        res = E.many_calls(bz, grid)
    finally:
        bz.close()
    pickle.dump(res, open(out_path, "wb"))


if __name__ == "__main__":
    {"lib": lib_step, "run": run_step, "many": many_step}[sys.argv[1]](*sys.argv[2:])
