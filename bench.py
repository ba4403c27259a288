#!/usr/bin/env python3
"""bench.py -- image-pairs/sec through the N-iter LM pose loop (BASELINE.json metric).

One "step" = one pass of the hot path over one synthetic batch already resident in HBM:
LM_S2GP.forward(sat, grd, mode='test') = two VGG16-U-Nets (MFMA convolutions) + 15 fused
projection/Jacobian/normal-equation/solve steps.  Workload at N=1: BASELINE configs[1]
(KITTI shapes, batch 32 per GPU, VGG-16 two-branch, 5 LM iters, 3-DoF, bf16).

    python bench.py --gpus 1 --steps 10 --warmup 3 [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

Multi-GPU: one process per GPU; the batch shards over ranks with no data-path collective
(every sample's solve is independent); a barrier + synchronize brackets the timed
region and the reported time is the MAX over ranks.  Prints ONE JSON line on rank 0.

A plain run sets up, runs W warm-up steps, times exactly K steps and prints the headline (`value`, `ms_per_step`).
--dump-outputs DIR writes what the last timed step returned -- the final pose of every pair, (shift_lat, shift_lon, theta)
or Ford's (shift_u, shift_v, theta) -- as DIR/<name>.npy (float32; N > 1: all ranks' shards in rank order).  The inputs and
weights are seeded, so two builds given the same arguments can be compared output for output.

With --full the line also carries the telemetry, per-kernel and roofline figures of the headline and, at N=1:
  by_precision   the same workload in each arithmetic mode -- fp32 (exact-fp32 MFMA), fp16x3 (split fp16, fp32-class
                 results) and bf16 -- with pairs/s, the dominant conv kernel's fraction of ITS roofline, and the measured
                 final-pose deviation from the reference's fp64 run on the committed golden inputs (tests/golden/), in
                 metres / radians, next to the north-star tolerance (1e-4 m / 1e-4 rad)
  secondary      short legs for BASELINE configs[3] (Ford, 10 LM iterations) and configs[4] (1024^2 / 512x2048, fp16)
  train          forward(train) + HIP backward + gradient all-reduce + Adam; train.by_precision: the same step in fp32 / fp16x3 / bf16
                 with the worst per-tensor relative L2 error and cosine of its gradients against the reference autograd
  cpu_baseline   the CPU oracle on this host's cores (bounded sample)
(--no-cpu-baseline, --no-kernel-timing, --no-extra-legs and --train-steps 0 trim a --full run.)
"""
import argparse
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

# dense peaks, /opt/skills/guides/MI355X_MICROARCH.md "Chip-level parameters".  fp16x3: every algorithmic FLOP costs three
# fp16 MFMA FLOPs, so the ceiling on ALGORITHMIC FLOPs is a third of the fp16 peak.
PEAK_TFLOPS = {'bf16': 2500.0, 'fp16': 2500.0, 'fp32': 157.3, 'fp16x3': 2500.0 / 3}
PEAK_HBM_GBS = 8000.0
from highlyaccurate_amd._s2gp import dead_ground_rows  # noqa: E402
from highlyaccurate_amd import synthetic  # noqa: E402

KITTI_K = [[582.9802, 0., 496.2420], [0., 482.7076, 125.0034], [0., 0., 1.]]     # models_kitti.py:657-660


def _cpu_model():
    try:
        for line in open('/proc/cpuinfo'):
            if line.startswith('model name'):
                return line.split(':', 1)[1].strip()
    except OSError:
        pass
    return 'unknown'


def cpu_baseline(budget_s=80.0):
    """The CPU oracle (oracle/ref_cpu.py, a port of the reference's PyTorch path; kind = "port") on THIS host's cores, as
    SURVEY 8(d) specifies it: KITTI shapes, fp32, B = 1 and B = 8 inference (forward(mode='test'), no_grad) and a B = 1
    training step (forward(mode='train') + backward), each on a bounded sample.  The torch thread count is PROBED on this host,
    separately for the single-pair and the batched forward (B = 1 and B = 4 passes over {16, 32, 64} threads; HLA_CPU_THREADS
    overrides), not assumed: on one MI355X host (256 logical CPUs) a B = 1 forward took 1.40 / 1.21 / 1.29 / 2.58 / 204 s with
    8 / 16 / 32 / 64 / 256 threads -- oversubscription kills it, and a batch can use more threads than a single pair."""
    from oracle import ref_cpu as O
    t_begin = time.time()
    ncpu = os.cpu_count() or 1
    net = O.build('kitti', O.default_args(), seed=1)
    sat, grd, gu, gv, gh = O.synth_images(101, 8)

    def fwd(B):
        t0 = time.time()
        with torch.no_grad():
            net(sat[:B], grd[:B], mode='test')
        return time.time() - t0

    if os.environ.get('HLA_CPU_THREADS'):
        cands = [min(ncpu, int(os.environ['HLA_CPU_THREADS']))]
    else:
        cands = sorted({min(ncpu, 16), min(ncpu, 32), min(ncpu, 64)})
    torch.set_num_threads(cands[0])
    fwd(1)                                              # warm-up (allocator, oneDNN primitives); not counted
    probe = {}
    for c in cands:
        torch.set_num_threads(c)
        probe[c] = fwd(1)
    cores = min(probe, key=probe.get)
    torch.set_num_threads(cores)
    # B = 1 inference: about 6 s of work
    reps = max(2, min(6, int(6.0 / max(probe[cores], 1e-3))))
    t1 = sum(fwd(1) for _ in range(reps))
    inf1 = reps / t1
    out = {'value': round(inf1, 4), 'unit': 'pairs/s', 'cores': cores, 'kind': 'port', 'host_cpus': ncpu, 'cpu_model': _cpu_model(),
           'thread_probe_s_per_pair': {str(k): round(v, 3) for k, v in probe.items()},
           'inference_b1': round(inf1, 4), 'inference_b8': None, 'training_b1': None}
    notes = [f'{reps} x B=1 forward(mode=test, no_grad) after 1 warm-up']
    # the batched forward gets its own probe (B = 4 passes, about 4 / inf1 seconds each): a batch parallelises over samples too
    cores8, probe8 = cores, {}
    for c in cands:
        if time.time() - t_begin + 4.0 / inf1 + 8.0 / inf1 > budget_s - 10.0:
            break
        torch.set_num_threads(c)
        probe8[c] = fwd(4) / 4.0
    if probe8:
        cores8 = min(probe8, key=probe8.get)
        out['thread_probe_b4_s_per_pair'] = {str(k): round(v, 3) for k, v in probe8.items()}
    torch.set_num_threads(cores8)
    est = 8.0 * (probe8[cores8] if probe8 else 1.0 / inf1)
    if time.time() - t_begin + est < budget_s:          # B = 8 inference: one pass (8 pairs)
        t8 = fwd(8)
        out['inference_b8'] = round(8.0 / t8, 4)
        out['cores_b8'] = cores8
        notes.append(f'1 x B=8 forward(mode=test, no_grad) on {cores8} threads')
    else:
        notes.append('B=8 skipped (would exceed the time budget)')
    torch.set_num_threads(cores)
    if time.time() - t_begin + 6.0 / inf1 < budget_s + 15.0:   # B = 1 training step: forward(train) + backward, one pass
        net.zero_grad(set_to_none=True)
        t0 = time.time()
        r = net(sat[:1], grd[:1], gu[:1], gv[:1], gh[:1], mode='train')
        r[0].backward()
        out['training_b1'] = round(1.0 / (time.time() - t0), 4)
        notes.append('1 x B=1 forward(mode=train) + backward')
    else:
        notes.append('training skipped (would exceed the time budget)')
    best_b8 = (out['inference_b8'] or 0.0) > out['inference_b1']
    out['value'] = out['inference_b8'] if best_b8 else out['inference_b1']        # the CPU's best inference rate ...
    out['cores'] = cores8 if best_b8 else cores                                   # ... and the threads THAT rate was measured on
    out['sample'] = ('KITTI shapes, fp32, 5 LM iters x 3 levels: ' + '; '.join(notes) +
                     f'; torch {torch.__version__} CPU, {cores} (B=1) / {cores8} (batched) of {ncpu} logical CPUs '
                     f'(probed over {cands}), {time.time() - t_begin:.0f} s in all')
    return out


# ---------------------------------------------------------------------------------------------------------------------
def build_net(model, precision, n_iters, dev, state=None):
    """Random-init weights of the reference architecture: Kaiming-normal(fan_out), zero bias (torchvision's non-pretrained
    VGG init; there is no network for the pretrained checkpoint) -- or a given state dict."""
    from highlyaccurate_amd.models_kitti import LM_G2SP, LM_S2GP
    from highlyaccurate_amd.models_ford import LM_S2GP_Ford
    args = synthetic.reference_args(N_iters=n_iters, precision=precision)
    torch.manual_seed(1234)                  # identical replicas on every rank (data-parallel training needs that)
    net = {'kitti': LM_S2GP, 'ford': LM_S2GP_Ford, 'g2sp': LM_G2SP}[model](args)
    if state is not None:
        net.load_state_dict(state)
    else:
        for m in net.modules():
            if isinstance(m, torch.nn.Conv2d):
                torch.nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
                if m.bias is not None:
                    torch.nn.init.zeros_(m.bias)
    return net.to(dev).eval()


def make_inputs(model, B, grd_hw, sat_a, dev, rank):
    torch.manual_seed(1234 + rank)           # a different synthetic shard per rank (also decorrelates the re-init draws)
    sat = torch.rand(B, 3, sat_a, sat_a, device=dev)
    grd = torch.rand(B, 3, grd_hw[0], grd_hw[1], device=dev)
    if model == 'ford':       # BASELINE configs[3] / SURVEY 8(d): fixed camera-to-body rotation, 112.64 m tile
        extra = (112.64, torch.tensor([[[0., 0., 1.], [1., 0., 0.], [0., 1., 0.]]], device=dev).repeat(B, 1, 1),
                 torch.tensor([[1.7, 0.3, -1.2]], device=dev).repeat(B, 1))
    elif model == 'g2sp':     # left_camera_k of the 256x1024 frame
        extra = (torch.tensor([KITTI_K], device=dev).repeat(B, 1, 1),)
    else:
        extra = ()
    return sat, grd, extra


def timed_infer(net, sat, grd, extra, steps, warmup, dist, tele=None):
    """W untimed steps, then exactly K steps bracketed by barrier + synchronize; MAX over ranks.  Returns (seconds, last output).
    tele: a Telemetry sampled over exactly the timed region (a side thread reading two sysfs files; nothing on the GPU)."""
    def step():
        with torch.no_grad():
            return net(sat, grd, *extra, mode='test')
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    if tele:
        tele.__enter__()
    t0 = time.perf_counter()
    out = None
    for _ in range(steps):
        out = step()
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if tele:
        tele.__exit__()
    if dist:
        tt = torch.tensor([dt], device=sat.device, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    return dt, out


OUTPUT_NAMES = {'kitti': ('shift_lat', 'shift_lon', 'theta'), 'g2sp': ('shift_lat', 'shift_lon', 'theta'),
                'ford': ('shift_u', 'shift_v', 'theta')}      # forward(mode='test')'s tuple, in order


def dump_outputs(path, model, out, dist):
    """--dump-outputs: `out` (one forward(mode='test') return value: B poses per rank, a few hundred bytes) as <path>/<name>.npy in
    float32 (float64 stays float64).  N > 1: every rank takes part in the gather, rank 0 writes the global batch in rank order."""
    arrs = [o.detach().to(torch.float64 if o.dtype == torch.float64 else torch.float32).cpu().numpy() for o in out]
    if dist:
        shards = [None] * dist.get_world_size()
        dist.all_gather_object(shards, arrs)
        if dist.get_rank() != 0:
            return
        arrs = [np.concatenate([s[i] for s in shards]) for i in range(len(arrs))]
    os.makedirs(path, exist_ok=True)
    for name, x in zip(OUTPUT_NAMES[model], arrs, strict=True):
        np.save(os.path.join(path, name + '.npy'), x)


def kernel_pass(net, sat, grd, extra, n):
    """The same step n more times with a HIP-event pair around every kernel launch (hla_prof_*, events recorded on the launch
    stream).  Kept out of `value`: the event pairs serialise kernel tails and cost ~9 % wall time."""
    from highlyaccurate_amd import _lib
    _lib.prof_enable(True)
    t1 = time.perf_counter()
    with torch.no_grad():
        for _ in range(n):
            net(sat, grd, *extra, mode='test')
    torch.cuda.synchronize()
    dt_ev = time.perf_counter() - t1
    _lib.prof_enable(False)
    return _lib.prof_fetch(), dt_ev


def aggregate(recs):
    agg = {}
    for name, ms, fl, by in recs:
        e = agg.setdefault(name, [0, 0.0, 0.0, 0.0])
        e[0] += 1; e[1] += ms; e[2] += fl; e[3] += by
    return agg


class Telemetry:
    """Shader clock (sclk) and socket power of ONE GPU, sampled from its hwmon sysfs files on a side thread (default 100 Hz;
    two small file reads per sample) while a timed region runs.  `roofline.peak` is the NOMINAL 2.5 PFLOP/s at 2.4 GHz; these
    fields say at what clock and power the timed region (and the mfma_sustained probe) actually ran, so that "0.5 of nominal =
    0.65-0.75 of what the chip sustains" can be checked by a reader who was not there (MI355X_MICROARCH.md, DVFS section)."""

    def __init__(self, device_index=0, hz=100.0):
        import threading
        self.dt = 1.0 / hz
        self.files = self._find(device_index)
        self.samples = []
        self._stop = threading.Event()
        self._th = None

    @staticmethod
    def _bus_id(device_index):
        try:
            pr = torch.cuda.get_device_properties(device_index)
            return f'{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}.0'
        except Exception:
            pass
        try:
            import ctypes
            hip = ctypes.CDLL('libamdhip64.so')
            buf = ctypes.create_string_buffer(32)
            if hip.hipDeviceGetPCIBusId(buf, 32, int(device_index)) == 0:
                return buf.value.decode().lower()
        except Exception:
            pass
        return None

    @classmethod
    def _find(cls, device_index):
        bus = cls._bus_id(device_index)
        cands = []
        for dev in sorted(glob.glob('/sys/class/drm/card*/device')):
            if bus and os.path.basename(os.path.realpath(dev)).lower() != bus:
                continue
            for hw in glob.glob(os.path.join(dev, 'hwmon', 'hwmon*')):
                f, pw = os.path.join(hw, 'freq1_input'), os.path.join(hw, 'power1_input')
                if not os.path.exists(pw):
                    pw = os.path.join(hw, 'power1_average')
                if os.path.exists(f) and os.path.exists(pw):
                    cands.append((f, pw))
        return cands[0] if len(cands) == 1 else None      # (ambiguous or absent: no telemetry rather than another GPU's)

    def _run(self):
        f, pw = self.files
        while not self._stop.is_set():
            try:
                self.samples.append((float(open(f).read()) / 1e6, float(open(pw).read()) / 1e6))
            except Exception:
                pass
            self._stop.wait(self.dt)

    def __enter__(self):
        import threading
        if self.files:
            self.samples, self._stop = [], threading.Event()
            self._th = threading.Thread(target=self._run, daemon=True)
            self._th.start()
        return self

    def __exit__(self, *exc):
        if self._th:
            self._stop.set()
            self._th.join()
            self._th = None

    def summary(self):
        """{'clock_mhz_mean', 'clock_mhz_min', 'power_w_mean', 'power_w_max', 'samples'} or {'samples': 0, 'why': ...}"""
        if not self.files:
            return {'samples': 0, 'why': 'no unambiguous hwmon freq1_input / power1_input for this device'}
        if not self.samples:
            return {'samples': 0, 'why': 'region shorter than one sampling period'}
        c, w = [x[0] for x in self.samples], [x[1] for x in self.samples]
        return {'clock_mhz_mean': round(sum(c) / len(c), 1), 'clock_mhz_min': round(min(c), 1), 'power_w_mean': round(sum(w) / len(w), 1),
                'power_w_max': round(max(w), 1), 'samples': len(c), 'source': 'hwmon freq1_input (sclk) / power1_input (socket), 100 Hz side thread'}


_PMC_SYMBOL = {'conv3x3_kernel<MT4,NT2>': 'Li4ELi2ELi2ELi2ELb0', 'conv3x3_kernel<MT4,NT2,pool>': 'Li4ELi2ELi2ELi2ELb1',
               'conv3x3_kernel<MT4,NT1>': 'Li4ELi1ELi2ELi2ELb0', 'conv3x3_kernel<MT4,NT1,pool>': 'Li4ELi1ELi2ELi2ELb1'}


def load_pmc():
    """HBM bytes per launch from the committed rocprofv3 PMC passes (tools/make_profiles.sh: separate --pmc FETCH_SIZE /
    --pmc WRITE_SIZE runs, gfx950 correction).  The file is stamped with the content hash of the kernel sources it was
    measured on; a file measured on OTHER kernels is ignored (traffic = null) instead of going silently stale."""
    from highlyaccurate_amd import _lib
    have = _lib.load().hla_source_hash().decode()
    for f in sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r*_pmc_hbm_traffic.json')), reverse=True):
        try:
            pm = json.load(open(f))
        except Exception:
            continue
        if pm.get('_source_hash') == have:
            return pm, os.path.relpath(f, ROOT)
    return None, None


def conv_roofline(agg, precision, pmc, pmc_src, headline_cfg):
    """The dominant FLOP-carrying kernel against the dense MFMA peak of its arithmetic."""
    dom = max((k for k in agg if agg[k][2] > 0), key=lambda k: agg[k][1])
    n, ms, fl, by = agg[dom]
    ach = fl / (ms * 1e-3) / 1e12
    traffic, tsrc = None, None
    sym = _PMC_SYMBOL.get(dom)
    if pmc and headline_cfg and sym:
        for kname, v in pmc.items():
            if isinstance(v, dict) and sym in kname and ('DF16b' in kname) == (precision == 'bf16'):
                traffic, tsrc = v['hbm_bytes_corrected'], pmc_src
    # (traffic: PMC passes need rocprofv3 around the process, so it comes from the committed file measured on the same kernel sources
    #  -- hash-checked --, and the line says so: traffic_measured_in_run)
    return {'kernel': dom, 'bound': 'mfma', 'achieved': round(ach, 2), 'peak': round(PEAK_TFLOPS[precision], 1),
            'unit': 'TFLOP/s', 'frac': round(ach / PEAK_TFLOPS[precision], 4), 'traffic': traffic,
            'traffic_unit': 'bytes/launch', 'traffic_source': tsrc,
            'traffic_measured_in_run': False, 'launches': n, 'avg_launch_us': round(ms / n * 1e3, 2),
            'flops_per_launch': round(fl / n / 1e9, 3), 'flops_unit': 'GFLOP (algorithmic: 2*9*Cin*Cout*pixels)'}


def mfma_sustained(precision, achieved):
    """roofline.peak is the NOMINAL dense MFMA peak (2.5 PFLOP/s at 2.4 GHz).  What the matrix pipe of this box sustains is
    measured here, in the same process: back-to-back MFMAs on register-resident operands (hla_prof_mfma_peak: no LDS, no memory,
    two waves per SIMD, ~8 ms) on zero operands, random operands and random operands with half the elements zero (post-ReLU-like).
    Only the first reaches the nominal figure; on real data the package power limit sets the rate, for ANY kernel."""
    from highlyaccurate_amd import _lib
    code = _lib.HLA_BF16 if precision == 'bf16' else _lib.HLA_F16
    div = 3.0 if precision == 'fp16x3' else 1.0            # three MFMAs per product (algorithmic FLOPs, like roofline.achieved)
    tele_out = {}
    try:
        tf = {}
        for k, d in (('zeros', 0), ('random', 1), ('random_half_zeros', 2)):
            # 150 ms per case: long enough for the power management to settle and for ~15 telemetry samples
            tl = Telemetry(torch.cuda.current_device())
            with tl:
                tf[k] = round(_lib.mfma_sustained_tflops(code, d, ms_target=150.0) / div, 1)
            tele_out[k] = {kk: vv for kk, vv in tl.summary().items() if kk != 'source'}
    except Exception as e:
        return {'error': repr(e)[:200]}
    return {'unit': 'TFLOP/s', **tf, 'frac_of_random_half_zeros': round(achieved / tf['random_half_zeros'], 4),
            'frac_of_random': round(achieved / tf['random'], 4), 'telemetry': tele_out,
            'what': 'hla_prof_mfma_peak: back-to-back v_mfma_f32_32x32x16 on register-resident operands, 2 waves/SIMD, all CUs, 150 ms '
                    'per case, measured in this run; the ceiling of any MFMA-bound kernel on this box on such data'}


def lm_roofline(agg, pmc, pmc_src):
    """The LM accumulate kernels against HBM.  `achieved` uses COUNTER bytes (what actually crossed the HBM interface per
    launch, committed PMC passes) over the live launch time; the algorithmic model (whole satellite map + ground half once
    per step) over-counts -- only the ground-plane footprint of the satellite map is touched and much of it is
    served by L2 / Infinity Cache -- so it is reported beside it, never as the achieved rate."""
    lm = [k for k in agg if k.startswith('lm_accum')]
    if not lm:
        return None
    ms = sum(agg[k][1] for k in lm)
    n = sum(agg[k][0] for k in lm)
    alg = sum(agg[k][3] for k in lm)
    out = {'kernel': 'lm_accum<*>', 'bound': 'hbm', 'peak': PEAK_HBM_GBS, 'unit': 'GB/s', 'launches': n,
           'avg_launch_us': round(ms / n * 1e3, 2), 'algorithmic_bytes_per_launch': round(alg / n),
           'algorithmic_gbs': round(alg / (ms * 1e-3) / 1e9, 1),
           'note': 'algorithmic_gbs is NOT an achieved bandwidth (the byte model counts the whole satellite map; a rate above the '
                   'HBM peak only means most of it never left the caches)'}
    cb = 0.0
    if pmc:
        for k in lm:
            C = k[len('lm_accum<'):-1]
            hit = [v for kn, v in pmc.items() if isinstance(v, dict) and (f'lm_accum<{C},' in kn or f'lm_accumILi{C}E' in kn)]
            if not hit:
                cb = None
                break
            cb += hit[0]['hbm_bytes_corrected'] * agg[k][0]
    else:
        cb = None
    if cb:
        ach = cb / (ms * 1e-3) / 1e9
        out.update({'achieved': round(ach, 1), 'frac': round(ach / PEAK_HBM_GBS, 4), 'traffic': round(cb / n),
                    'traffic_unit': 'bytes/launch (counter)', 'traffic_source': pmc_src, 'traffic_measured_in_run': False,
                    'traffic_over_algorithmic': round(cb / alg, 3)})
    else:
        out.update({'achieved': None, 'frac': None, 'traffic': None})
    return out


def pose_deviation(precision, dev, model='kitti'):
    """Final pose of the golden inputs in this arithmetic mode, as the worst deviation from the reference's fp64 run in metres /
    radians, next to the reference's own fp32-vs-fp64 gap and the parity gate of SURVEY 8(c): |ours - ref64| <= max(tol, 2 |ref32 - ref64|).
    model = 'kitti': tests/golden/e2e_kitti.npz (4 seeds x B=2, full KITTI shapes, 15 LM steps; recorded from the REAL reference in
    fp32 and fp64); 'ford': e2e_ford.npz (BASELINE configs[3]: 2 seeds, 30 LM steps); 'hires': e2e_kitti_hires.npz (configs[4] sizes,
    30 LM steps)."""
    fname = {'kitti': 'e2e_kitti.npz', 'ford': 'e2e_ford.npz', 'hires': 'e2e_kitti_hires.npz'}[model]
    g = np.load(os.path.join(ROOT, 'tests', 'golden', fname), allow_pickle=False)
    B = int(g['B'])
    to_m, to_rad = 20.0, 10.0 * np.pi / 180.0                     # shift_range_lat/lon, rotation_range (reference defaults)
    tol = np.array([1e-4 / to_m, 1e-4 / to_m, 1e-4 / to_rad])
    dev_m = dev_rad = gap_m = gap_rad = 0.0
    worst = 0.0
    seeds = [int(g['seed'])] if model == 'hires' else [int(s) for s in g['seeds']]
    for seed in seeds:
        kind, n_it = ('ford', 10) if model == 'ford' else ('kitti', 10 if model == 'hires' else 5)
        net = build_net(kind, precision, n_it, dev, state=synthetic.model_state(seed))
        hw, sa = ((512, 2048), 1024) if model == 'hires' else ((256, 1024), 512)
        sat, grd, *_ = synthetic.images(seed + 100, B, grd_hw=hw, sat_a=sa)
        extra = ()
        if model == 'ford':
            extra = (112.64, torch.tensor([[[0., 0., 1.], [1., 0., 0.], [0., 1., 0.]]], device=dev).repeat(B, 1, 1),
                     torch.tensor([[1.7, 0.3, -1.2]], device=dev).repeat(B, 1))
        torch.manual_seed(seed)
        with torch.no_grad():
            net(sat.to(dev), grd.to(dev), *extra, mode='test')
        ours = net.last_trace.reshape(B, -1, 3)[:, -1].double().cpu().numpy()     # final (shift_u, shift_v, theta)
        sfx = '' if model == 'hires' else f'_{seed}'
        r64, r32 = g['trace64' + sfx][:, -1], g['trace32' + sfx][:, -1]
        e, gap = np.abs(ours - r64), np.abs(r32 - r64)
        dev_m, dev_rad = max(dev_m, e[:, :2].max() * to_m), max(dev_rad, e[:, 2].max() * to_rad)
        gap_m, gap_rad = max(gap_m, gap[:, :2].max() * to_m), max(gap_rad, gap[:, 2].max() * to_rad)
        worst = max(worst, (e / np.maximum(tol, 2 * gap)).max())
        del net
    return {'final_pose_dev_shift_m': float(f'{dev_m:.3e}'), 'final_pose_dev_yaw_rad': float(f'{dev_rad:.3e}'),
            'reference_fp32_vs_fp64_shift_m': float(f'{gap_m:.3e}'), 'reference_fp32_vs_fp64_yaw_rad': float(f'{gap_rad:.3e}'),
            'tolerance': '1e-4 m / 1e-4 rad (north_star)', 'gate_ratio': round(float(worst), 3),
            'meets_parity_gate': bool(worst <= 1.0),
            'inputs': f'tests/golden/{fname}: {len(seeds)} seed(s) x {B} pairs, ' +
                      {'kitti': 'full KITTI shapes, 15 LM steps', 'ford': 'Ford shapes, 30 LM steps',
                       'hires': 'sat 1024 / grd 512x2048, 30 LM steps'}[model]}


def gradient_fidelity(precision, dev):
    """One training step on the committed golden input (tests/golden/train_kitti.npz: full KITTI shape, B = 1; gradient samples
    recorded from the REAL reference's autograd in fp64 and fp32) in this arithmetic mode: per tensor the relative L2 error and
    the cosine of our gradient against the reference's fp64 gradient on the recorded sample positions (64 per tensor, 7 tensors
    from both branches, encoder to decoder), worst over the tensors, next to the reference's own fp32-vs-fp64 figures."""
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'train_kitti.npz'), allow_pickle=False)
    seed, B = int(g['seed']), int(g['B'])
    net = build_net('kitti', precision, 5, dev, state=synthetic.model_state(seed)).train()
    sat, grd, gu, gv, gh = synthetic.images(seed + 100, B)
    torch.manual_seed(seed)
    r = net(sat.to(dev), grd.to(dev), gu.to(dev), gv.to(dev), gh.to(dev), mode='train')
    r[0].backward()
    named = dict(net.named_parameters())
    worst_l2, worst_cos, ref_l2, worst_key = 0.0, 1.0, 0.0, ''
    for k in [k[len('grad64_'):] for k in g.files if k.startswith('grad64_')]:
        ref, r32 = g['grad64_' + k][2:], g['grad32_' + k][2:]
        gr = named[k].grad.double().reshape(-1).cpu().numpy()
        got = gr[synthetic.fixture_sample_idx(gr.size, 77)]
        l2 = float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))
        cos = float(np.dot(got, ref) / max(np.linalg.norm(got) * np.linalg.norm(ref), 1e-300))
        ref_l2 = max(ref_l2, float(np.linalg.norm(r32 - ref) / max(np.linalg.norm(ref), 1e-300)))
        if l2 > worst_l2:
            worst_l2, worst_key = l2, k
        worst_cos = min(worst_cos, cos)
    loss_rel = abs(float(r[0].detach()) - float(g['tuple64'][0][0])) / abs(float(g['tuple64'][0][0]))
    return {'worst_rel_l2': float(f'{worst_l2:.3e}'), 'worst_tensor': worst_key, 'worst_cosine': round(worst_cos, 9),
            'reference_fp32_vs_fp64_worst_rel_l2': float(f'{ref_l2:.3e}'), 'loss_rel_err': float(f'{loss_rel:.3e}'),
            'inputs': 'tests/golden/train_kitti.npz: 7 tensors x 64 sampled gradient elements of the reference autograd (fp64), full KITTI shape, B = 1'}


def workload_name(model, sat_a, grd_hw, n_iters):
    base = {'kitti': ("BASELINE configs[1]: LM_S2GP" if (sat_a, tuple(grd_hw)) == (512, (256, 1024)) else "BASELINE configs[4] sizes: LM_S2GP"),
            'ford': "BASELINE configs[3] shapes: LM_S2GP_Ford", 'g2sp': "SURVEY 8(f).2: LM_G2SP"}[model]
    return (base + f".forward(mode='test'), sat {sat_a}x{sat_a}, grd {grd_hw[0]}x{grd_hw[1]}, VGG-16 two-branch, level 3, "
            f"{n_iters} LM iters x 3 levels, 3-DoF, random-init weights")


def step_breakdown(tstep, nsteps, dist=None, sync=None):
    """Phase times of a training step from HIP events recorded on the launch (current) stream at the phase boundaries the model
    marks (``_s2gp.PHASE_HOOK``): the two extractor forwards, the LM loop, `glue` (the pose loss forward + its backward, i.e.
    everything between the LM loop and the model's backward), the LM backward (incl. the zero-fills in front of it), both
    extractors' backward (the satellite one on a side stream, joined before the mark), the optimizer -- and `inter_step_idle`:
    the time between the optimizer's last kernel and the first mark of the NEXT step, which is zero when the host runs ahead of the
    GPU and the host's lateness otherwise.  Medians over the steps; `sum` is the median event-to-event step time,
    `host_enqueue_ms` the host time one step's launches take (no sync inside)."""
    from highlyaccurate_amd import _s2gp
    order = ['fwd_sat', 'fwd_grd', 'lm_fwd', 'loss', 'lm_bwd', 'vgg_bwd', 'optimizer']
    steps, cur, host = [], [], []

    def hook(name):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        cur.append((name, ev))

    tstep()                      # (one untimed step: whatever the previous block left behind is flushed)
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    _s2gp.PHASE_HOOK = hook
    if sync is not None:
        sync.timing, sync._timeline = True, []
    try:
        for _ in range(nsteps + 1):
            cur = []
            t0 = time.perf_counter()
            hook('begin')
            tstep()
            hook('optimizer')
            host.append(time.perf_counter() - t0)
            steps.append(cur)
        torch.cuda.synchronize()
    finally:
        _s2gp.PHASE_HOOK = None
        if sync is not None:
            sync.timing = False
    overlap = sync.overlap_report() if sync is not None else []
    rows = []
    for i in range(nsteps):
        ev = dict(steps[i])
        if any(k not in ev for k in order):       # (a model that does not mark its phases, e.g. LM_G2SP)
            continue
        r, prev = {}, ev['begin']
        for k in order:
            r[k] = prev.elapsed_time(ev[k])
            prev = ev[k]
        r['inter_step_idle'] = ev['optimizer'].elapsed_time(dict(steps[i + 1])['begin'])
        r['sum'] = ev['begin'].elapsed_time(dict(steps[i + 1])['begin'])
        rows.append(r)
    out = {'_steps_run': nsteps + 2}
    if not rows:
        return dict(out, error='the model marks no phases')
    med = lambda k: round(float(np.median([r[k] for r in rows])), 3)
    out.update({'unit': 'ms', 'steps': len(rows), 'fwd_sat': med('fwd_sat'), 'fwd_grd': med('fwd_grd'), 'lm_fwd': med('lm_fwd'),
                'glue': med('loss'), 'lm_bwd': med('lm_bwd'), 'vgg_bwd': med('vgg_bwd'), 'optimizer': med('optimizer'),
                'inter_step_idle': med('inter_step_idle'), 'sum': med('sum'),
                'host_enqueue_ms': round(float(np.median(host[:-1])) * 1e3, 3),
                'what': 'HIP events on the launch stream at the phase marks (median over the steps of a block that is not part of value); '
                        'fwd_sat includes the weight repacking after the optimizer step; vgg_bwd = both extractors (two streams, joined)'})
    if overlap:      # N > 1 (or the forced one-rank group): how much of the gradient all-reduce the backward did NOT cover
        ov = overlap[:nsteps]
        out['allreduce_exposed_ms'] = round(float(np.median([o['exposed_ms'] for o in ov])), 3)
        nb = min(len(o['bucket_issue_ms_before_backward_end']) for o in ov)
        out['allreduce_buckets'] = [{'bytes': ov[0]['bucket_bytes'][k],
                                     'issued_ms_before_backward_end': round(float(np.median([o['bucket_issue_ms_before_backward_end'][k] for o in ov])), 3)}
                                    for k in range(nb)]
        out['allreduce_what'] = ('events on the launch stream: a bucket is issued when its branch\'s weight gradients are complete; '
                                 'exposed = from the first wait (the whole backward is enqueued behind it) to the last collective returning')
    return out


def train_leg(net, a, sat, grd, extra, B, world, rank, dist, dev, want_kt, extras=True):
    from highlyaccurate_amd import _lib
    from highlyaccurate_amd.parallel import GradSync
    net.train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    gt = [torch.rand(B, 1, device=dev) * 2 - 1 for _ in range(3)]
    if a.model == 'ford':      # Ford_dataset.py:211 collates python floats: [B] float64
        gt = [g[:, 0].double() for g in gt]

    def tstep(o=None):
        o = o or opt
        o.zero_grad(set_to_none=True)
        r = net(sat, grd, *extra, gt[0], gt[1], gt[2], mode='train')
        r[0].backward()
        o.step()
        return r[0]

    def timed(nsteps, warm=2):
        for _ in range(warm):       # warm-up: Adam state, caching-allocator segments for the backward workspaces
            tstep()
        torch.cuda.synchronize()
        if dist:
            dist.barrier()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        lossv = None
        for _ in range(nsteps):
            lossv = tstep()
        torch.cuda.synchronize()
        if dist:
            dist.barrier()
        torch.cuda.synchronize()
        tdt = time.perf_counter() - t1
        if dist:
            tt = torch.tensor([tdt], device=dev, dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            tdt = float(tt.item())
        return tdt, lossv

    # N > 1: rank 0 first times the SAME step alone (no gradient exchange, the other ranks wait at a barrier), so that the line
    # can state what the all-reduce costs: train.scaling_eff = train.value / (N x that single-rank rate), both measured here
    single = None
    if dist:
        if rank == 0:
            opt0 = torch.optim.Adam(net.parameters(), lr=0.0)    # the same work, but the replica stays identical to the others'
            for _ in range(2):
                tstep(opt0)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(a.train_steps):
                tstep(opt0)
            torch.cuda.synchronize()
            single = B * a.train_steps / (time.perf_counter() - t1)
            del opt0
        dist.barrier()
        net.grad_sync = GradSync(force=True)       # (force: also in HLA_BENCH_FORCE_DIST's one-rank group)
    ar0 = net.grad_sync.bytes_reduced if dist else 0
    # Three timed blocks of K steps; `value` is the MEDIAN block and all three are in the line (train.blocks_ms_per_step; the
    # fastest as best_block_ms_per_step).  On a fresh box one block in ~10 runs came out at twice the step time of every other
    # block of the same process (profiles/r03: 48.1 ms against 22.5-23.7 ms before and after it; a one-off stall of ~0.15 s
    # inside six steps, not a property of the step): the median ignores one such block without reporting a best-of.
    tdts = []
    tele = Telemetry(torch.cuda.current_device()) if rank == 0 else None
    for blk in range(3):
        # (four warm-up steps, round 5: with two, the first block of a fresh process came out 2-47 % slower than the other two --
        #  Adam state, the caching allocator's backward-workspace segments on BOTH streams, and the clocks settling)
        tb, lossv = timed(a.train_steps, warm=4) if blk == 0 else timed(a.train_steps, warm=0)
        tdts.append(tb)
    blocks = [round(t / a.train_steps * 1e3, 3) for t in tdts]
    tdt = sorted(tdts)[1]
    # clock / power: sampled over a FOURTH block of the same steps that is not part of `value`, so that the sampler cannot be
    # suspected of what the blocks show.  (In full default runs the MIDDLE block comes out 8-35 % slow -- [47.2, 58.4, 47.7],
    # [48.0, 52.6, 48.7] ms -- with the sampler in it or not; a process that runs this leg alone on a cool chip shows
    # [47.0, 47.5, 47.7], and tools/probes/telemetry_ab.py measures no effect of the sampler on either leg: it is the chip's
    # power management after the preceding legs, and the median is there for it.)
    # (EVERY rank runs the block -- a step contains the gradient all-reduce and `timed` its barriers -- only rank 0 samples)
    if tele:
        tele.__enter__()
    tb4, _ = timed(a.train_steps, warm=0)
    if tele:
        tele.__exit__()
    tele_block = round(tb4 / a.train_steps * 1e3, 3)
    # ---- where the step goes: events on the launch stream at the phase boundaries (highlyaccurate_amd._s2gp.PHASE_HOOK), a block
    # of its own, not part of `value`.  Every rank runs it (the step contains the all-reduce), rank 0 reports.
    breakdown = step_breakdown(tstep, max(3, min(a.train_steps, 6)), dist, getattr(net, 'grad_sync', None) if dist else None)
    n_bd = breakdown.pop('_steps_run')
    ar_bytes = ((net.grad_sync.bytes_reduced - ar0) // (4 * a.train_steps + 4 + n_bd)) if dist else 0      # 3 timed blocks + the telemetry block of K steps + 4 warm-up steps + the breakdown block
    trecs = []
    if not a.no_kernel_timing:  # per-kernel table from two extra steps (not part of the timing).  EVERY rank runs them --
        if want_kt:             # a training step contains the gradient all-reduce -- but only rank 0 is instrumented
            _lib.prof_enable(True)
        for _ in range(2):
            tstep()
        torch.cuda.synchronize()
        if want_kt:
            _lib.prof_enable(False)
            trecs = _lib.prof_fetch()
    live = None
    if a.model != 'g2sp' and extras:       # one more step with the backward's diagnostics on: which share of its tiles the satellite branch visits
        net.bwd_stats = {}
        tstep()
        torch.cuda.synchronize()
        st, net.bwd_stats = net.bwd_stats, None
        if st.get('total_tiles'):
            live = round(st['live_tiles'] / st['total_tiles'], 3)
    if dist:
        dist.barrier()
    train = {'value': round(B * world * a.train_steps / tdt, 3), 'unit': 'pairs/s', 'steps': a.train_steps,
             'ms_per_step': round(tdt / a.train_steps * 1e3, 3), 'blocks_ms_per_step': blocks, 'value_is': 'median of 3 blocks',
             'best_block_ms_per_step': min(blocks), 'loss_finite': bool(torch.isfinite(lossv)),
             'what': "forward(mode='train') + HIP backward (LM loop + both VGGs) + gradient all-reduce + Adam",
             'allreduce_bytes_per_step': ar_bytes, 'step_breakdown': breakdown,
             'sat_backward_live_tiles': live}       # data-dependent trimming; None = dense walk
    if dist:
        train['single_rank_value'] = round(single, 3) if single else None      # rank 0 alone, same step, no all-reduce
        train['scaling_eff'] = round(train['value'] / (world * single), 4) if single else None
    if a.model != 'g2sp' and extras:
        # secondary number: the same step with args.train_ground_crop=1 (an extension: the ground branch trains on the
        # image rows that can reach the loss; loss and gradients equal to rounding, the RETURNED confidence maps are
        # only computed from the crop on -- DESIGN.md 3.5).  Not the default, so it is not `train.value`.
        net.args.train_ground_crop = 1
        cdt, _ = timed(a.train_steps)
        net.args.train_ground_crop = 0
        train['with_train_ground_crop'] = {'value': round(B * world * a.train_steps / cdt, 3), 'unit': 'pairs/s',
                                           'ms_per_step': round(cdt / a.train_steps * 1e3, 3)}
    if tele:
        train['telemetry'] = dict(tele.summary(), block_ms_per_step=tele_block,
                                  what='a fourth block of the same steps, sampled; not part of value')
    if trecs:
        tagg = aggregate(trecs)
        tot = sum(v[1] for v in tagg.values())
        # The step against the MFMA roofline, on EXECUTED FLOPs: every conv / dgrad / wgrad launch logs 2*9*Cin*Cout*pixels for
        # the rows it computes, and a data-dependent launch of the backward (satellite branch: only the tiles whose gradient is
        # not exactly zero) logs the share of its tiles it visited (hla_prof_begin_dyn).  `achieved` = those FLOPs of ONE step
        # over the un-instrumented step time of train.value; peak = the dense MFMA peak of the step's arithmetic (fp16x3:
        # 2500 / 3 TFLOP/s of algorithmic FLOPs -- three MFMAs per product).
        prec = getattr(net.args, 'precision', 'fp32')
        fl_step = sum(v[2] for v in tagg.values()) / 2.0          # two instrumented steps
        ach = fl_step / (tdt / a.train_steps) / 1e12
        train['gflop_per_pair_executed'] = round(fl_step / B / 1e9, 2)
        train['roofline'] = {'bound': 'mfma', 'achieved': round(ach, 2), 'peak': round(PEAK_TFLOPS[prec], 1), 'unit': 'TFLOP/s',
                             'frac': round(ach / PEAK_TFLOPS[prec], 4),
                             'flops': 'executed: forward(train) convs + data gradients + weight gradients of one step, trimmed rows / tiles excluded',
                             'by_kernel_tflops_instrumented': {k: round(v[2] / (v[1] * 1e-3) / 1e12, 1) for k, v in tagg.items() if v[2] > 0}}
        # (no TFLOP/s here: the backward skips the tiles whose gradient is exactly zero -- data-dependent, DESIGN.md 6 -- so
        #  the FLOPs a dgrad / wgrad launch executes are not the dense layer's; per-launch numbers: tools/probes/train_launches.py)
        train['kernels'] = {k: {'launches': v[0], 'avg_us': round(v[1] / v[0] * 1e3, 1), 'share': round(v[1] / tot, 3)}
                            for k, v in sorted(tagg.items(), key=lambda kv: -kv[1][1])[:8]}
    net.eval()
    return train


def _free_port():
    import socket
    with socket.socket() as so:
        so.bind(('127.0.0.1', 0))
        return so.getsockname()[1]


def launcher_command(n_ranks, argv, port):
    """The command `python bench.py --gpus N` re-executes itself under when it was started WITHOUT a launcher: one process
    per GPU, rendezvous on 127.0.0.1 (the container hostname may not resolve) -- the same line the driver uses."""
    return [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={n_ranks}',
            '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__), *argv]


def self_launch(n_ranks, argv):
    import subprocess
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')     # dmabuf IPC: RCCL needs it on this driver
    env.setdefault('OMP_NUM_THREADS', '8')
    env['HLA_BENCH_SELF_LAUNCHED'] = '1'
    return subprocess.run(launcher_command(n_ranks, argv, _free_port()), env=env).returncode


def resolve_world(gpus, environ):
    """(world, rank, local_rank) of THIS process, or None when the process still has to spawn its ranks.  `--gpus N` is the
    contract: it must equal the launcher's WORLD_SIZE; a plain `python bench.py --gpus N` (no launcher) spawns N ranks."""
    if 'WORLD_SIZE' not in environ:
        if gpus > 1:
            return None
        return 1, 0, 0
    world = int(environ['WORLD_SIZE'])
    if world != gpus:
        raise SystemExit(f'bench.py: --gpus {gpus} but the launcher started WORLD_SIZE={world} ranks; they must agree '
                         f'(n_gpus in the JSON line is the number of ranks that really ran)')
    return world, int(environ.get('RANK', '0')), int(environ.get('LOCAL_RANK', '0'))


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--batch', type=int, default=32, help='pairs per GPU')
    ap.add_argument('--precision', default='bf16', choices=['bf16', 'fp16', 'fp32', 'fp16x3'])
    ap.add_argument('--n-iters', type=int, default=None, help='LM iterations (default 5; 10 for --model ford = BASELINE configs[3])')
    ap.add_argument('--grd-hw', type=int, nargs=2, default=[256, 1024], help='ground image size (BASELINE configs[4]: 512 2048)')
    ap.add_argument('--sat-a', type=int, default=512, help='satellite image side (BASELINE configs[4]: 1024)')
    ap.add_argument('--model', default='kitti', choices=['kitti', 'ford', 'g2sp'],
                    help='kitti = LM_S2GP (the headline, BASELINE configs[1]); ford = LM_S2GP_Ford; g2sp = LM_G2SP')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help="write the last timed step's outputs as DIR/<name>.npy (float32)")
    ap.add_argument('--full', action='store_true',
                    help='besides the headline, run every other measurement and check of the line (telemetry, per-kernel timing and '
                         'rooflines, training step, other precisions and configs, accuracy against the goldens, CPU baseline); '
                         'the --no-* / --train-* options below apply to such a run')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-kernel-timing', action='store_true')
    ap.add_argument('--no-extra-legs', action='store_true', help='skip by_precision and the secondary configs (N=1 extras)')
    ap.add_argument('--train-steps', type=int, default=6, help='extra: time this many training steps (0 = skip)')
    ap.add_argument('--train-precision', default='fp16x3', choices=['bf16', 'fp16', 'fp32', 'fp16x3'],
                    help="arithmetic mode of the `train` object (default fp16x3: the fastest mode whose gradients match the reference's "
                         "autograd inside the fp32 gates; bf16 / fp16 steps are reported under train.by_precision as non-parity extras)")
    a = ap.parse_args(argv)
    if a.steps < 1 or a.warmup < 0:
        ap.error('--steps must be >= 1 and --warmup >= 0')
    if a.n_iters is None:
        a.n_iters = 10 if a.model == 'ford' else 5

    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')    # (also when a launcher started us: before the first HIP call)
    wr = resolve_world(a.gpus, os.environ)
    if wr is None:                       # `python bench.py --gpus N` with no launcher: be the launcher
        sys.exit(self_launch(a.gpus, argv))
    world, rank, local = wr
    assert torch.cuda.is_available(), 'bench.py needs an MI355X'
    # Fewer GPUs than ranks (HLA_BENCH_REHEARSE=1, or detected): REHEARSAL -- the ranks share devices and the collectives go over
    # gloo instead of RCCL.  It checks the multi-rank control flow only; the line says "rehearsal": true and its numbers are not
    # a scaling measurement.
    ndev = torch.cuda.device_count()
    rehearse = bool(os.environ.get('HLA_BENCH_REHEARSE')) or world > ndev
    if rehearse:
        if rank == 0:
            print(f'bench.py: REHEARSAL -- {world} ranks on {ndev} GPU(s), gloo instead of RCCL; not a scaling measurement',
                  file=sys.stderr, flush=True)
        local %= ndev
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    dist = None
    ranks_seen = 1
    # HLA_BENCH_FORCE_DIST=1 (test hook): run the N = 1 job through the process group too -- RCCL with one rank -- so that every
    # collective call of the N > 1 path (barriers, MAX over ranks, the gradient all-reduce inside the backward) executes on RCCL on
    # a 1-GPU box; tests/test_gpu_parity.py::test_bench_single_rank_through_rccl
    force_dist = bool(os.environ.get('HLA_BENCH_FORCE_DIST')) and world == 1
    if world > 1 or force_dist:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        if force_dist:
            os.environ.setdefault('MASTER_PORT', str(_free_port()))
        if rehearse:
            dist.init_process_group('gloo', rank=rank, world_size=world)
        else:
            dist.init_process_group('nccl', rank=rank, world_size=world, device_id=dev)
        # proof that the collective backend really spans N ranks: every rank contributes 1 (and its device index)
        one = torch.ones(2, device=dev, dtype=torch.float64)
        one[1] = float(torch.cuda.current_device())
        dist.all_reduce(one, op=dist.ReduceOp.SUM)
        ranks_seen = int(one[0].item())

    from highlyaccurate_amd import _lib
    _lib.load()
    B = a.batch
    net = build_net(a.model, a.precision, a.n_iters, dev)
    sat, grd, extra = make_inputs(a.model, B, a.grd_hw, a.sat_a, dev, rank)
    want_kt = (rank == 0) and a.full and not a.no_kernel_timing

    # ---- the timed region: exactly K steps, no instrumentation
    tele = Telemetry(local) if rank == 0 and a.full else None
    dt, out = timed_infer(net, sat, grd, extra, a.steps, a.warmup, dist, None)
    if a.dump_outputs:
        dump_outputs(a.dump_outputs, a.model, out, dist)
    if a.full:
        # clock / power of the headline: sampled over a SEPARATE block of the same steps that lasts >= 1 s (>= 100 samples at 100 Hz)
        # and is not part of `value` -- the timed region itself is 0.1-0.3 s, 13 samples, not a steady-state reading (VERDICT r05 #8a).
        # N > 1: every rank runs the block (timed_infer has barriers), rank 0 samples.
        n_tele = max(a.steps, int(1.2 / max(dt / a.steps, 1e-4)) + 1)
        dt_tele, _ = timed_infer(net, sat, grd, extra, n_tele, 0, dist, tele)
    # ---- the same steps once more on rank 0 with a HIP-event pair around every kernel launch: per-kernel durations for the
    # rooflines.  Kept out of `value` (measured: 8.73 vs 7.97 ms/step), and it would make rank 0 the slowest rank of every multi-GPU run.
    recs, dt_ev = [], None
    n_ev = min(a.steps, 50)               # bound the instrumented pass (130 event pairs per step)
    if want_kt:
        recs, dt_ev = kernel_pass(net, sat, grd, extra, n_ev)
    if dist:
        dist.barrier()
    if not os.environ.get('HLA_BENCH_NOCHECK'):     # timing-ablation library builds (tools/ab_libs.py) produce garbage
        assert all(torch.isfinite(o).all() for o in out)

    headline_cfg = (a.model == 'kitti' and B == 32 and a.sat_a == 512 and tuple(a.grd_hw) == (256, 1024) and a.n_iters == 5)
    pmc, pmc_src = load_pmc() if rank == 0 and a.full else (None, None)

    # ---- extra: the training step (forward(train) + HIP backward + gradient all-reduce + Adam), same shapes
    train = None
    if a.full and a.train_steps > 0:
        # train.value is measured in the mode whose GRADIENTS are the reference's (the bf16 step's gradients differ
        # from the reference autograd by 0.24 relative L2, the fp16 step's by 0.077 -- the 16-bit dgrad / wgrad products' own
        # rounding, amplified by the cancellation in these gradient sums; the same figures come out behind an exact forward, and
        # gradient scaling changes nothing: DESIGN 6, tools/probes/mixed_bwd_fidelity.py): --train-precision, default fp16x3.
        # The bf16 / fp16 steps stay in the line as train.by_precision entries marked parity_grade: false.
        try:
            tnet = net if a.train_precision == a.precision else build_net(a.model, a.train_precision, a.n_iters, dev)
            train = train_leg(tnet, a, sat, grd, extra, B, world, rank, dist, dev, want_kt)
            train['dtype'] = a.train_precision
            train['parity_grade'] = a.train_precision in ('fp32', 'fp16x3')
            if tnet is not net:
                del tnet
                torch.cuda.empty_cache()
        except Exception as e:      # the headline line must still be printed
            train = {'error': repr(e)[:300]}

    # ---- N=1: the training step in every arithmetic mode -- pairs/s and the fidelity of its gradients against the reference's
    # autograd (the reference trains in fp32: 'fp16x3' is the mode that matches it, on split-fp16 dgrad / wgrad kernels)
    if train and 'error' not in train and world == 1 and headline_cfg and not a.no_extra_legs:
        tbp = {}
        for p in ('fp32', 'fp16x3', 'fp16', 'bf16'):
            try:
                if p == a.train_precision:
                    e = {'value': train['value'], 'ms_per_step': train['ms_per_step'], 'steps': train['steps']}
                    if 'roofline' in train:
                        e['roofline'] = {k_: train['roofline'][k_] for k_ in ('bound', 'achieved', 'peak', 'unit', 'frac')}
                        e['gflop_per_pair_executed'] = train['gflop_per_pair_executed']
                else:
                    net = None
                    torch.cuda.empty_cache()
                    net = build_net('kitti', p, 5, dev)
                    sub = argparse.Namespace(**vars(a))
                    sub.train_steps, sub.no_kernel_timing = (3 if p == 'fp32' else 4), a.no_kernel_timing
                    t2 = train_leg(net, sub, sat, grd, extra, B, 1, 0, None, dev, want_kt, extras=False)
                    e = {'value': t2['value'], 'ms_per_step': t2['ms_per_step'], 'steps': t2['steps'], 'blocks_ms_per_step': t2['blocks_ms_per_step']}
                    if 'roofline' in t2:
                        e['roofline'] = {k_: t2['roofline'][k_] for k_ in ('bound', 'achieved', 'peak', 'unit', 'frac')}
                        e['gflop_per_pair_executed'] = t2['gflop_per_pair_executed']
                e['unit'] = 'pairs/s'
                e['gradients'] = gradient_fidelity(p, dev)
                e['parity_grade'] = p in ('fp32', 'fp16x3')      # gradients inside the fp32 gates of the reference-autograd goldens
                tbp[p] = e
            except Exception as ex:
                tbp[p] = {'error': repr(ex)[:300]}
        train['by_precision'] = tbp
        net = None
        torch.cuda.empty_cache()
        net = build_net(a.model, a.precision, a.n_iters, dev)

    # ---- N=1 extras: the other arithmetic modes on the same workload, and BASELINE configs[3] / [4]
    by_precision, secondary = None, None
    if a.full and world == 1 and headline_cfg and not a.no_extra_legs:
        by_precision = {}
        for p in ('fp32', 'fp16x3', 'bf16', 'fp16'):     # (fp16: the dtype configs[4] names, on configs[1]'s workload)
            try:
                if p == a.precision:
                    e = {'value': round(B * a.steps / dt, 3), 'ms_per_step': round(dt / a.steps * 1e3, 3), 'steps': a.steps}
                    prec_recs = recs
                else:
                    net = None
                    torch.cuda.empty_cache()
                    net = build_net('kitti', p, 5, dev)
                    k = 10 if p == 'fp32' else 20
                    # (three blocks of k steps, the MEDIAN one counts, all are reported: these short secondary legs run right after
                    #  a new library module was first used; one-off stalls of tens of ms showed up in them on fresh boxes)
                    pdts = []
                    for blk in range(3):
                        pb, pout = timed_infer(net, sat, grd, extra, k, 3 if blk == 0 else 0, None)
                        pdts.append(pb)
                    assert all(torch.isfinite(o).all() for o in pout)
                    blocks = [round(t / k * 1e3, 3) for t in pdts]
                    pdt = sorted(pdts)[1]
                    e = {'value': round(B * k / pdt, 3), 'ms_per_step': round(pdt / k * 1e3, 3), 'steps': k, 'blocks_ms_per_step': blocks,
                         'value_is': 'median of 3 blocks'}
                    prec_recs = kernel_pass(net, sat, grd, extra, 5)[0] if not a.no_kernel_timing else []
                e['unit'] = 'pairs/s'
                if prec_recs:
                    r = conv_roofline(aggregate(prec_recs), p, None, None, False)
                    e['roofline'] = {k_: r[k_] for k_ in ('kernel', 'bound', 'achieved', 'peak', 'unit', 'frac', 'avg_launch_us')}
                e['accuracy'] = pose_deviation(p, dev)
                by_precision[p] = e
            except Exception as ex:
                by_precision[p] = {'error': repr(ex)[:300]}
        secondary = {}
        # every leg in the dtype its config names AND in fp16x3 (the matched-accuracy mode), each with the final-pose deviation of
        # that mode on the config's golden inputs (VERDICT r05 #6b: both legs used to be reported only in dtypes that miss 1e-4 m)
        for tag, gold, kw in (('configs[3] Ford', 'ford', dict(model='ford', precision='bf16', n_iters=10, B=32, grd_hw=(256, 1024), sat_a=512, steps=15)),
                              ('configs[4] hires fp16', 'hires', dict(model='kitti', precision='fp16', n_iters=10, B=8, grd_hw=(512, 2048), sat_a=1024, steps=10))):
            for prec in (kw['precision'], 'fp16x3'):
                key = tag if prec == kw['precision'] else tag.replace(' fp16', '') + ' fp16x3'
                try:
                    net = None
                    torch.cuda.empty_cache()
                    net = build_net(kw['model'], prec, kw['n_iters'], dev)
                    s2, g2, x2 = make_inputs(kw['model'], kw['B'], kw['grd_hw'], kw['sat_a'], dev, rank)
                    nst = kw['steps'] if prec != 'fp16x3' else max(4, kw['steps'] // 2)
                    sdts = []
                    for blk in range(3):      # (three blocks, the median counts, as for by_precision above)
                        sb, sout = timed_infer(net, s2, g2, x2, nst, 5 if blk == 0 else 0, None)
                        sdts.append(sb)
                    sblocks = [round(t / nst * 1e3, 3) for t in sdts]
                    sdt = sorted(sdts)[1]
                    secondary[key] = {'value': round(kw['B'] * nst / sdt, 3), 'unit': 'pairs/s', 'dtype': prec,
                                      'ms_per_step': round(sdt / nst * 1e3, 3), 'blocks_ms_per_step': sblocks, 'value_is': 'median of 3 blocks',
                                      'steps': nst, 'pairs_per_gpu': kw['B'],
                                      'finite': bool(all(torch.isfinite(o).all() for o in sout)),
                                      'workload': workload_name(kw['model'], kw['sat_a'], kw['grd_hw'], kw['n_iters'])}
                    del s2, g2, x2
                    net = None
                    torch.cuda.empty_cache()
                    secondary[key]['accuracy'] = pose_deviation(prec, dev, gold)
                except Exception as ex:
                    secondary[key] = {'error': repr(ex)[:300]}

    if rank == 0:
        pairs = B * world * a.steps
        res = {
            'metric': 'image-pairs/sec through N-iter LM pose loop, KITTI shapes',
            'value': round(pairs / dt, 3), 'unit': 'pairs/s', 'n_gpus': world, 'steps': a.steps, 'warmup': a.warmup,
            'ms_per_step': round(dt / a.steps * 1e3, 3), 'higher_is_better': True, 'scaling': 'weak',
            'vs_baseline': None, 'dtype': a.precision, 'data': 'synthetic',
            'config': {'workload': workload_name(a.model, a.sat_a, a.grd_hw, a.n_iters),
                       'pairs_per_gpu': B, 'global_batch': B * world, 'parallelism': f'batch-sharded x{world}, no collective',
                       'dead_work_skipped': 'dec3/conf3 (VGG.py:153-155,163: computed and dropped by the reference at level 3); '
                                            f'ground-image rows 0..{dead_ground_rows(grd.shape[-2]) - 1} (cannot reach the bottom-half '
                                            'rows the LM loop reads) and, layer by layer, the feature rows those rows do not '
                                            'depend on; computed rows are bit-identical, DESIGN.md 3.5)'},
        }
        if dist:
            res['collective_ranks_seen'] = ranks_seen      # all-reduced count over the process group (RCCL unless rehearsing)
            res['collective_backend'] = 'gloo (rehearsal)' if rehearse else 'nccl (RCCL)'
            res['rehearsal'] = rehearse                     # true: the ranks SHARE GPUs -- control-flow check, not a measurement
            res['n_gpus_physical'] = min(world, ndev)
            res['self_launched'] = bool(os.environ.get('HLA_BENCH_SELF_LAUNCHED'))
            res['scale_reads'] = ('value = inference pairs/s, batch sharded over the ranks, no data-path collective (weak scaling, '
                                  f'{B} pairs per GPU); train.value = data-parallel training pairs/s INCLUDING the gradient '
                                  'all-reduce over RCCL (train.allreduce_bytes_per_step, train.scaling_eff)')
        if recs:
            agg = aggregate(recs)
            # whole-forward conv rate on the FLOPs that were actually EXECUTED (dead rows / dead layers excluded; the
            # reference's as-written count is 316.3 GFLOP/pair, 272.4 without dec3/conf3)
            conv_fl = sum(v[2] for k, v in agg.items() if k.startswith('conv'))      # over the n_ev instrumented steps
            res['conv_gflop_per_pair_executed'] = round(conv_fl / (B * n_ev) / 1e9, 2)
            res['conv_tflops_executed'] = round(conv_fl / n_ev * a.steps / dt / 1e12, 2)   # this GPU, against the un-instrumented time
            tot_ms = sum(v[1] for v in agg.values())
            res['events_pass_ms_per_step'] = round(dt_ev / n_ev * 1e3, 3)
            res['roofline'] = conv_roofline(agg, a.precision, pmc, pmc_src, headline_cfg)
            # clock and power of the TIMED region (and, inside mfma_sustained, of each probe case): VERDICT r04 #5
            ts = tele.summary() if tele else {'samples': 0}
            ts = dict(ts, block_steps=n_tele, block_ms_per_step=round(dt_tele / n_tele * 1e3, 3),
                      what='a separate block of the same steps (>= 1 s), sampled; not part of value')
            res['roofline']['clock_mhz_mean'] = ts.get('clock_mhz_mean')
            res['roofline']['power_w_mean'] = ts.get('power_w_mean')
            res['roofline']['telemetry'] = ts
            if a.precision in ('bf16', 'fp16', 'fp16x3'):
                ms_ = mfma_sustained(a.precision, res['roofline']['achieved'])
                res['roofline']['mfma_sustained'] = ms_
                probe = (ms_.get('telemetry') or {}).get('random_half_zeros') or {}
                res['roofline']['mfma_sustained_clock_mhz_mean'] = probe.get('clock_mhz_mean')
                res['roofline']['mfma_sustained_power_w_mean'] = probe.get('power_w_mean')
            lmr = lm_roofline(agg, pmc if headline_cfg else None, pmc_src)
            if lmr:
                res['lm_roofline'] = lmr
            res['kernels'] = {k: {'launches': v[0], 'avg_us': round(v[1] / v[0] * 1e3, 2), 'share': round(v[1] / tot_ms, 4),
                                  'tflops': round(v[2] / (v[1] * 1e-3) / 1e12, 2) if v[2] else None}
                              for k, v in sorted(agg.items(), key=lambda kv: -kv[1][1])}
        if by_precision:
            res['by_precision'] = by_precision
            ma = by_precision.get('fp16x3') or {}
            if 'value' in ma:
                # the number that satisfies north_star's "1e-4 m / 1e-4 rad" on this workload, next to `value` (which is the dtype
                # BASELINE configs[1] names, bf16: NOT at that accuracy -- by_precision.bf16.accuracy)
                acc = ma.get('accuracy') or {}
                res['matched_accuracy'] = {'dtype': 'fp16x3', 'value': ma['value'], 'unit': 'pairs/s', 'ms_per_step': ma['ms_per_step'],
                                           'roofline_frac': (ma.get('roofline') or {}).get('frac'),
                                           'roofline_peak_tflops': PEAK_TFLOPS['fp16x3'],
                                           'final_pose_dev_shift_m': acc.get('final_pose_dev_shift_m'),
                                           'final_pose_dev_yaw_rad': acc.get('final_pose_dev_yaw_rad'),
                                           'meets_parity_gate': acc.get('meets_parity_gate'),
                                           'headline_dtype_meets_parity_gate': ((by_precision.get(a.precision) or {}).get('accuracy') or {}).get('meets_parity_gate')}
        if secondary:
            res['secondary'] = secondary
        if train:
            res['train'] = train
        if a.full and not a.no_cpu_baseline and world == 1:        # rank 0 at N = 1 only (the task's contract)
            try:
                res['cpu_baseline'] = cpu_baseline()
            except Exception as ex:     # the headline line must still be printed
                res['cpu_baseline'] = {'error': repr(ex)[:300]}
        print(json.dumps(res), flush=True)
    if dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
