"""Stage-1 wall time (6 calls, best) on the C2 assembly for lines that take the GENERAL path of count_kernel, which none of
tools/stage1_time.py's does: windows of 17 - 32 positions (64-bit registers) in the three strand modes, `both` with a
non-palindromic pattern of 7 ones (16 384 bins: no second histogram, so no fast path), more than four runs (generic run loop)."""
import sys, time
import numpy as np, torch
sys.path.insert(0, '.')
import phyloligo_amd as pa
from phyloligo_amd import synthetic
ctx = pa.Context(0)
seq, off = synthetic.contig_bytes(50000, 2000, seed=50001)
dseq = torch.from_numpy(seq).cuda(); doff = torch.from_numpy(off.astype(np.int64)).cuda()
for pattern, strand in (("10000000000000000101", "both"), ("1100000000000000011", "plus"), ("11000000000000000000011", "minus"),
                        ("11011111", "both"), ("1010101011", "plus"), ("10110100000000000000001", "both")):
    b = 1e9
    for _ in range(6):
        torch.cuda.synchronize(); t = time.perf_counter()
        c, tt = ctx.count_profiles(dseq, doff, pattern, strand)
        torch.cuda.synchronize(); b = min(b, time.perf_counter() - t)
    print("C2 %-24s %-5s %8.1f us  sum %d" % (pattern, strand, b * 1e6, int(tt.sum())), flush=True)
    del c, tt
