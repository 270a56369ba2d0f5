"""Child process of tests/test_gpu_bamsort.py: one GPU step, under the time limit the parent sets.
    bamsort_gpu_run.py lib <out.pkl>      test_bamsort_emul.vectors() through libstaramd.so's sorter at levels 1 and 6
    bamsort_gpu_run.py many <out.pkl>     one finish of 2 x CUs x 3 + 5 blocks of short records: more output tiles than k_bamsort_gather has workgroups
                                          (4 per CU, 32 KiB each), more blocks than k_bgzf_blocks has (2 per CU)"""
import hashlib
import os
import pickle
import random
import sys
import time
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from util import capi  # noqa: E402
import test_bamsort_emul as S  # noqa: E402
import test_bgzf_emul as E  # noqa: E402


def lib_step(out_path):
    bz = capi.BgzfDevice(device=0)
    try:
        got = {(lv, name): S.sort_vector(bz, None, vec, lv)[0] for lv in (1, 6) for name, vec in S.vectors().items()}
    finally:
        bz.close()
    pickle.dump(got, open(out_path, "wb"))


def many_step(out_path):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nb = 2 * cus * 3 + 5
    total = nb * S.IN_MAX - 1234
    r = random.Random(7)
    pool = [S._record(r, i, r.randint(40, 160)) for i in range(997)]
    appends, recs, keys, size, i = [], [], [], 0, 0
    while size < total:
        data, ks = bytearray(), []
        while len(ks) < 150000 and size < total:
            rec = pool[i % 997][:total - size]
            ks.append((r.randrange(1 << 12) << 32 | r.randrange(1 << 16), i % 3, len(data), len(rec)))
            data += rec; size += len(rec); i += 1
        appends.append((bytes(data), ks))
        recs += [data[o:o + n] for _, _, o, n in ks]; keys += [(g, x) for g, x, _, _ in ks]
    order = sorted(range(len(recs)), key=lambda j: (keys[j][0], keys[j][1], j))
    want = b"".join(recs[j] for j in order)
    assert len(want) == total
    bz = capi.BgzfDevice(device=0)
    bs = capi.BamSortDevice(bz)
    try:
        for data, ks in appends:
            assert bs.append(data, ks)
        t0 = time.time()
        out = bs.finish(1)
        seconds, stats = time.time() - t0, bs.stats
        ref = bz.compress(1, [want])[0]
    finally:
        bs.close()
        bz.close()
    inflated, p = [], 0
    while p < len(out):                                             # (the framing of every member is checked on the vectors; here the content)
        bsize = int.from_bytes(out[p + 16:p + 18], "little") + 1
        inflated.append(zlib.decompress(out[p + 18:p + bsize - 8], -15))
        p += bsize
    pickle.dump({"cus": cus, "nb": nb, "blocks": len(inflated), "records": len(recs), "bytes": total, "seconds": seconds, "stats": stats, "same_as_compressor": out == ref,
                 "content": hashlib.sha256(b"".join(inflated)).hexdigest() == hashlib.sha256(want).hexdigest(),
                 "isize": all(len(x) == S.IN_MAX for x in inflated[:-1])}, open(out_path, "wb"))


if __name__ == "__main__":
    {"lib": lib_step, "many": many_step}[sys.argv[1]](*sys.argv[2:])
