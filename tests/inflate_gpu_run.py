"""Child process of tests/test_gpu_inflate.py: one GPU step, under the time limit the parent sets.
    inflate_gpu_run.py lib <out.pkl>     every vector of tests/inflate_vectors.py through libstaramd.so (staramd_inflate_host_file)
    inflate_gpu_run.py sweep <out.pkl>   3 x (grid cap) + 5 members of seven kinds with STARAMD_INFLATE_MAX_WORKGROUPS=6, so that the grid-stride loop turns and every
                                         wavefront meets several kinds; every member also alone, before and after the large call"""
import os
import pickle
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from util import capi  # noqa: E402
import inflate_vectors as V  # noqa: E402

SWEEP_WORKGROUPS = 6


def lib_step(out_path):
    d = capi.InflateDevice()
    got = {"constants": (d.workgroup, d.members_per_workgroup, d.workgroups_per_cu, d.max_workgroups())}
    for name, (f, _) in V.wellformed().items():
        got[("well", name)] = d.host_file(f)
    for name, (f, _, _) in list(V.malformed().items()) + list(V.lenient().items()):
        got[("bad", name)] = d.host_file(f)[:3]
    for name, (f, _) in V.not_bgzf().items():
        try:
            d.host_file(f)
            got[("not", name)] = None
        except RuntimeError as e:
            got[("not", name)] = str(e)
    pickle.dump(got, open(out_path, "wb"))


def sweep_members(n):
    import test_inflate_emul as E
    return E.many_members(n)


def sweep_step(out_path):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    os.environ["STARAMD_INFLATE_MAX_WORKGROUPS"] = str(SWEEP_WORKGROUPS)
    d = capi.InflateDevice()
    cap = min(d.max_workgroups(), d.workgroups_per_cu * cus) * d.members_per_workgroup
    ms = sweep_members(3 * cap + 5)
    got = {"cus": cus, "cap": cap, "n": len(ms)}
    got["before"] = [d.host_file(m)[0] for m in ms]
    got["all"] = d.host_file(b"".join(ms))
    got["after"] = [d.host_file(m)[0] for m in ms]
    pickle.dump(got, open(out_path, "wb"))


if __name__ == "__main__":
    {"lib": lib_step, "sweep": sweep_step}[sys.argv[1]](*sys.argv[2:])
