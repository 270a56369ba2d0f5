"""Child process of tests/test_gpu_dedup.py: one GPU step, under the time limit the parent sets.
    dedup_gpu_run.py lib <out.pkl> <bits | ->   test_dedup_emul.vectors() through libstaramd.so (staramd_dedup_host_records) for every option set, with
                                                STARAMD_DEDUP_HASH_BITS=<bits> when given
    dedup_gpu_run.py sweep <out.pkl>            `many` and `deep` with STARAMD_DEDUP_MAX_WORKGROUPS=8, so that every grid-stride loop turns many times; reports
                                                the CU count and the grid cap in force"""
import os
import pickle
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from util import capi  # noqa: E402
import test_dedup_emul as D  # noqa: E402

SWEEP_WORKGROUPS = 8


def lib_step(out_path, bits):
    if bits != "-":
        os.environ["STARAMD_DEDUP_HASH_BITS"] = bits
    dd = capi.DedupDevice()
    got = {"constants": (dd.workgroup, dd.workgroups_per_cu, dd.max_workgroups())}
    for name, recs in D.vectors().items():
        for opt in D.options(name):
            got[(name, opt)] = D.result_of(dd.host_records(recs, *opt))
    pickle.dump(got, open(out_path, "wb"))


def sweep_step(out_path):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    os.environ["STARAMD_DEDUP_MAX_WORKGROUPS"] = str(SWEEP_WORKGROUPS)
    dd = capi.DedupDevice()
    got = {"cus": cus, "workgroups": min(dd.max_workgroups(), dd.workgroups_per_cu * cus), "tile": dd.workgroup}
    for name in ("many", "deep"):
        for opt in D.OPTION_SETS:
            got[(name, opt)] = D.result_of(dd.host_records(D.vectors()[name], *opt))
    pickle.dump(got, open(out_path, "wb"))


if __name__ == "__main__":
    {"lib": lib_step, "sweep": sweep_step}[sys.argv[1]](*sys.argv[2:])
