"""K0 + K1 of the bench workload on their own (10 000 images x 512 channels x 4x4, 16 drop layers), three rotating input
sets: HIP-event time of K0, of K1 from its table, and of the one launch that reads the draws itself (mc_entropy_lut_kernel,
the product form), interleaved in one loop; the profiling target of the `rocprofv3 --pmc` passes in profiles/.
  python3 tools/k1_probe.py [--iters 300] [--repeats 3] [--counter]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from runia_core_amd import _hip
if os.environ.get('RUNIA_LIB'):  # an ablation build of the library (tools/ablate)
    _hip._LIB_PATH = os.environ['RUNIA_LIB']

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=300)
ap.add_argument("--repeats", type=int, default=1)
ap.add_argument("--counter", action="store_true")
ap.add_argument("--warm", type=float, default=0.5)
a = ap.parse_args()
dev = torch.device("cuda", 0)
n, n_mc = 10000, 16
sets = [bench.synth_latents(n, 1235 + 1000 * j, 0.0, dev) for j in range(3)]
lib = _hip.load_library()
wsb = int(lib.runia_mc_entropy_workspace_bytes(n, 4, 4, n_mc))
ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
h = torch.empty(n, 512, dtype=torch.float64, device=dev)
h_lut = torch.empty_like(h)
lut_t = _hip._flag_lut(dev, 4, 4, 2)
st = torch.cuda.current_stream().cuda_stream

def k0(j, i):
    x, r = sets[j]
    if a.counter:
        rc = lib.runia_mc_mask_table_counter_f32(7, i * n, ws.data_ptr(), wsb, n, 4, 4, n_mc, 0.5, 2, st)
    else:
        rc = lib.runia_mc_mask_table_f32(r.data_ptr(), n_mc * 16, ws.data_ptr(), wsb, n, 4, 4, n_mc, 0.5, 2, st)
    assert rc == 0

def k1(j):
    x, _ = sets[j]
    rc = lib.runia_mc_entropy_from_table_f32(x.data_ptr(), ws.data_ptr(), wsb, h.data_ptr(), None, None, n, 512, 4, 4, n_mc, 5, 1e-5, st)
    assert rc == 0

def k1_lut(j):
    x, r = sets[j]
    rc = lib.runia_mc_entropy_lut_f32(x.data_ptr(), r.data_ptr(), n_mc * 16, lut_t.data_ptr(), lut_t.numel() * 4, h_lut.data_ptr(), None,
                                      n, 512, 4, 4, n_mc, 0.5, 2, 5, 1e-5, st)
    assert rc == 0

t0 = time.perf_counter()
while time.perf_counter() - t0 < a.warm:
    for i in range(30):
        k0(i % 3, i); k1(i % 3); k1_lut(i % 3)
    torch.cuda.synchronize()
import numpy as np
# the two forms never read the same set back to back (a launch would find the other's latent maps in the Infinity Cache): the
# q-th map-reading launch takes set q % 3, so two other sets, 676 MB, pass between two reads of a set
for rep in range(a.repeats):
    ev = [tuple(torch.cuda.Event(enable_timing=True) for _ in range(4)) for _ in range(a.iters)]
    for i in range(a.iters):
        e0, e1, e2, e3 = ev[i]
        e0.record(); k0((2 * i) % 3, i); e1.record(); k1((2 * i) % 3); e2.record(); k1_lut((2 * i + 1) % 3); e3.record()
    torch.cuda.synchronize()
    if not a.counter:  # the last table launch's set through both forms, for the comparison below
        k0(0, 0); k1(0); k1_lut(0)
        torch.cuda.synchronize()
    t_k0 = np.array([e[0].elapsed_time(e[1]) for e in ev]); t_k1 = np.array([e[1].elapsed_time(e[2]) for e in ev])
    t_lut = np.array([e[2].elapsed_time(e[3]) for e in ev]); t_sum = t_k0 + t_k1
    same = "n/a (counter draws)" if a.counter else bool(torch.equal(torch.nan_to_num(h), torch.nan_to_num(h_lut)))
    print(f"K0 median {np.median(t_k0) * 1e3:.1f} us   K1 median {np.median(t_k1) * 1e3:.1f} us  (min {t_k1.min() * 1e3:.1f}, p90 {np.percentile(t_k1, 90) * 1e3:.1f})  "
          f"K0 + K1 median {np.median(t_sum) * 1e3:.1f} us  (min {t_sum.min() * 1e3:.1f})   "
          f"K1 from draws median {np.median(t_lut) * 1e3:.1f} us  (min {t_lut.min() * 1e3:.1f}, p90 {np.percentile(t_lut, 90) * 1e3:.1f})  "
          f"equal {same}  checksum {float(torch.nan_to_num(h).sum()):.6f}")
