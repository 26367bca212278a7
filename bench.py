"""Headline benchmark: images/sec of the student-teacher training step on synthetic COCO-shaped batches.

    python bench.py --gpus N --steps K --warmup W           (N=1 directly)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

One process per GPU (RCCL), 2 images per GPU (weak scaling), fp32.  Every step takes a batch that a staging thread
copied from pinned host memory on its own stream while earlier steps computed (data/prefetch.py::DevicePrefetcher; the
reference moves every batch inside its loop, engine/trainer.py:103-107) -- the copy of step k+2 is in flight under step
k, so the batch IS resident when its step starts; ``--resident-input`` re-uses one device batch instead (A/B).  A step is
forward (frozen trunk + teacher pseudo-labelling + two student passes) -> backward with the bucketed
gradient all-reduce overlapped -> SGD.  Rank 0 prints ONE JSON line with the fields the driver reads.  A plain run
does only what that headline needs: set-up, clock warm-up, W warm-up steps, the K timed steps, the outputs of the last
timed step when ``--dump-outputs DIR`` is given (DIR/<name>.npy: every loss term, and a seeded sample of every trainable
parameter's gradient), the line.  ``--full`` adds
  replay       : a few sequential steps after the timed region, for the per-kernel figures below;
  secondary    : a short timed region of the teacher configuration (student workload only, --secondary-steps);
  roofline     : the hand-written kernel the step spends most time in (the pair-layout split GEMM of the res5
                 head / frozen trunk: matrix-core bound, bf16 MFMA flops issued / HIP-event time against the
                 2.5 PFLOP/s dense bf16 peak; a byte kernel would be priced against the 8 TB/s HBM peak),
                 measured with HIP events on the launch stream (sequential replay when the step is pipelined);
  kernels      : the same for every native op that ran;
  config.roi_align_856MB : the one-second RoIAlign micro-benchmark (N=1);
  cpu_baseline : the reference's own CPU kernels (oracle/_ref; falls back to the C port) on the native-op
                 work of ONE image of the same step, on the host cores (N=1, rank 0 only).
Without ``--full`` those fields are null (``kernels`` empty, ``replay_steps`` 0) and ``cpu_baseline`` is absent.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on this driver: RCCL between ranks needs it


def _spawn_if_asked():
    """``python bench.py --gpus N`` with N > 1 and no launcher environment: this process becomes the launcher -- it starts
    N children (one per GPU, env:// rendezvous on 127.0.0.1, the same command line), relays rank 0's JSON line through
    its own stdout and exits with the job's code.  It runs BEFORE torch is imported: the parent never touches the GPU
    and nothing is exec'ed over a process that has (engine/launch.py)."""
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import launch

    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument("--gpus", type=int, default=1)
    known, _ = pre.parse_known_args()
    if launch.needs_spawn(known.gpus):
        sys.exit(launch.spawn_ranks([os.path.abspath(__file__)] + sys.argv[1:], known.gpus))
    # a rank: pin it to its share of the cores (of its GPU's NUMA node when sysfs tells) BEFORE torch / HIP start any
    # thread -- the runtime's helper threads and the trainer's worker thread inherit the mask
    return launch.apply_rank_affinity()


AFFINITY = {"cpus": None, "source": "not applied (imported as a module)"}
if __name__ == "__main__":
    AFFINITY = _spawn_if_asked()

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8 TB/s spec
IMS_PER_GPU = 2


MFMA_BF16_PEAK_TFLOPS = 2500.0  # same guide: dense bf16 matrix peak (the 2:1-sparsity figure is never used)
MFMA_F32_PEAK_TFLOPS = 157.3    # same guide: fp32-input matrix peak (= the fp32 vector peak)
MFMA_SUSTAINED_TFLOPS = 1540.0  # measured: MFMAs + fragment reads of the split GEMM loop without any loads


class OpTimer:
    """HIP-event timing of the native ops on the stream they are launched on (torch's current stream).  Every op is
    recorded with its ALGORITHMIC work: bytes for the HBM-bound byte kernels, matrix-core flops for the split GEMMs
    (three bf16 products of 2*M*N*K flops each per fp32-accurate product; fp32-equivalent rate = a third of it)."""

    def __init__(self, C):
        self.C = C
        self.records = {}   # name -> list of (start_event, end_event, work)
        self.kind = {}      # name -> "hbm" | "mfma"
        self.bytes = {}     # name -> algorithmic HBM bytes of the matrix-core ops (every operand / result once)
        self.enabled = False
        self._orig = {}

    def _wrap(self, name, work_fn, kind="hbm", bytes_fn=None, shape_fn=None):
        orig = getattr(self.C, name)
        self._orig[name] = orig
        self.kind[name] = kind
        self.bytes.setdefault(name, 0.0)

        def wrapped(*args, **kwargs):
            if not self.enabled:
                return orig(*args, **kwargs)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = orig(*args, **kwargs)
            b.record()
            self.records.setdefault(name, []).append((a, b, work_fn(*args, **kwargs),
                                                      shape_fn(*args, **kwargs) if shape_fn else None))
            if bytes_fn is not None:
                self.bytes[name] += bytes_fn(*args, **kwargs)
            return out

        setattr(self.C, name, wrapped)

    def install(self):
        def roi_fwd_bytes(inp, rois, scale, ph, pw, sr):
            n, c, h, w = inp.shape
            return 4 * rois.shape[0] * c * ph * pw + 4 * n * c * h * w + 20 * rois.shape[0]

        def roi_bwd_bytes(grad, rois, scale, ph, pw, n, c, h, w, sr):
            return 4 * rois.shape[0] * c * ph * pw + 4 * n * c * h * w + 20 * rois.shape[0]

        def nms_bytes(dets, scores, thr, ge_mode=False):
            k = dets.shape[0]
            nb = (k + 63) // 64
            return 20 * k + 2 * 8 * k * nb + 8 * k

        def split_bytes(x, mode):
            return 10 * x.numel()  # 4 B read + 3 x 2 B written per element

        def im2col_bytes(x, kh, kw, flip=False):
            return (4 + 6 * kh * kw) * x.numel()  # source once + [hi | hi | lo] for every tap

        def bias_act_bytes(y, bias=None, residual=None, relu=True):
            return (8 + (4 if residual is not None else 0)) * y.numel()

        def roi_fwd_strided_bytes(inp, rois, scale, ph, pw, sr, bs):
            n, c, h, w = inp.shape
            return 4 * rois.shape[0] * c * (-(-ph // bs)) * (-(-pw // bs)) + 4 * n * c * h * w + 20 * rois.shape[0]

        def split_pair_bytes(x):
            return 8 * x.numel()  # 4 B read + hi + lo written

        def gate_split_bytes(dy, gate=None, want_f32=False, pooled=None, pool_rows=0, selected=None, group_slot=None):
            n = dy.numel() if dy is not None else pooled.numel() * pool_rows
            per = (4 if dy is not None else 0) + 4 + (0 if gate is None else (2 if gate.dtype == torch.bfloat16 else 4))
            return ((per + (4 if want_f32 else 0)) * n + (0 if pooled is None else 4 * pooled.numel())
                    + (0 if selected is None else 4 * selected.numel() + 4 * group_slot.numel()))

        def split_gemm_flops(a_pair, b_pair, *args, **kwargs):
            return 6.0 * a_pair.shape[0] * b_pair.shape[0] * (b_pair.shape[1] // 2)  # 3 products x 2*M*N*K

        def split_gemm_bytes(a_pair, b_pair, bias=None, residual=None, relu=False, out_f32=True, out_pair=False, **kwargs):
            # every operand once: A and B pair rows (4 B / value), the fp32 and / or pair result, the shortcut
            m, n = a_pair.shape[0], b_pair.shape[0]
            return (2 * a_pair.numel() + 2 * b_pair.numel() + 4 * m * n * (int(bool(out_f32)) + int(bool(out_pair)))
                    + (4 * m * n if (residual is not None or kwargs.get("residual_pair") is not None) else 0))

        def split_gemm_gated_bytes(a_pair, b_pair, gate_pair, conv=None, out_f32=False, out_pair=True):
            m, n = a_pair.shape[0], b_pair.shape[0]
            return 2 * a_pair.numel() + 2 * b_pair.numel() + 4 * m * n * (int(bool(out_f32)) + int(bool(out_pair))) + 2 * m * n

        def split_gemm_rp_gated_bytes(a_pair, b_pair, residual_pair, gate_pair, out_f32=False, out_pair=True):
            m, n = a_pair.shape[0], b_pair.shape[0]  # operands, the pair shortcut (4 B / value), the gate's hi halves (2 B), results
            return (2 * a_pair.numel() + 2 * b_pair.numel() + 4 * m * n * (int(bool(out_f32)) + int(bool(out_pair))) + 4 * m * n
                    + 2 * m * n)

        def split_gemm_tn_bytes(g_pair, x_pair, conv=None, scale=None, weight_shape=None):
            taps = 1 if conv is None else conv[2] * conv[3]
            return 2 * g_pair.numel() + 2 * x_pair.numel() + 4 * (g_pair.shape[1] // 2) * (x_pair.shape[1] // 2) * taps

        def split_gemm_tn_flops(g_pair, x_pair, conv=None, scale=None, weight_shape=None):
            taps = 1 if conv is None else conv[2] * conv[3]
            return 6.0 * g_pair.shape[0] * (g_pair.shape[1] // 2) * (x_pair.shape[1] // 2) * taps

        self._wrap("roi_align_forward", roi_fwd_bytes)
        self._wrap("roi_align_forward_mfma", roi_fwd_bytes)
        self._wrap("roi_align_forward_strided_nhwc", roi_fwd_strided_bytes)
        self._wrap("roi_align_forward_strided_pair", roi_fwd_strided_bytes)
        self._wrap("roi_align_backward", roi_bwd_bytes)

        def roi_bwd_strided_bytes(grad, rois, scale, ph, pw, n, c, h, w, sr, bs):
            return 4 * grad.numel() + 4 * n * c * h * w + 20 * rois.shape[0]  # the computed bins' tiles + the planes

        self._wrap("roi_align_backward_strided", roi_bwd_strided_bytes)
        self._wrap("roi_align_backward_strided_nhwc", roi_bwd_strided_bytes)  # same bytes: the NHWC gradient + the planes
        self._wrap("nms_padded", nms_bytes)

        def nms_batched_bytes(boxes, drop, threshold, below=0, ge_mode=False):
            n, k = boxes.shape[0], boxes.shape[1]
            nb = (k + 63) // 64
            return n * (16 * k + (4 * k if drop is not None else 0) + 8 * k * (nb + 1) // 2 * 2 + 8 * k)  # boxes, flags, upper-triangle mask written + read, keep

        def rpn_decode_bytes(box_regression, topk_idx, cell_anchors, image_wh, weights, xform_clip, min_size, anchor_stride):
            return topk_idx.numel() * (8 + 16 + 16 + 4)  # index + 4 deltas read, box + flag written

        self._wrap("nms_presorted_batched", nms_batched_bytes)
        self._wrap("rpn_decode", rpn_decode_bytes)
        self._wrap("split_bf16x3", split_bytes)
        self._wrap("im2col_split_bf16x3", im2col_bytes)
        self._wrap("bias_act_", bias_act_bytes)
        self._wrap("split_pair", split_pair_bytes)
        self._wrap("gate_split_pair", gate_split_bytes)
        def nt_shape(a_pair, b_pair, *args, conv=None, **kwargs):
            taps = 1 if conv is None else conv[2] * conv[3]
            return (a_pair.shape[0], b_pair.shape[0], b_pair.shape[1] // 2, taps)

        def tn_shape(g_pair, x_pair, conv=None, scale=None, weight_shape=None):
            taps = 1 if conv is None else conv[2] * conv[3]
            return (g_pair.shape[0], g_pair.shape[1] // 2, x_pair.shape[1] // 2 * taps, taps)

        def gemm_nt_flops(a, b, bias=None):
            return 2.0 * a.shape[0] * b.shape[0] * a.shape[1]  # exact-fp32 matrix-core GEMM: 2*M*N*K

        def gemm_nt_bytes(a, b, bias=None):
            return 4 * (a.numel() + b.numel() + a.shape[0] * b.shape[0])

        def align_bytes(region_emb, noun_emb):
            return 4 * (region_emb.numel() + noun_emb.numel()) + 12 * noun_emb.shape[0]

        def ce_bytes(logits, labels, bg_weight, need_grad=True):
            return 4 * logits.numel() * (2 if need_grad else 1) + 8 * labels.numel()

        def bce_bytes(mu, sigma, eps, pos_index, targets, channel, need_grad=True):
            p = pos_index.numel()
            px = targets.numel() // max(p, 1)
            per = 2 + (2 if sigma is not None else 0) + (2 if need_grad else 0)  # mu/eps channels read, gradients written
            return 4 * p * px * (per + 1) + 8 * p

        def box_decode_bytes(rel_codes, boxes, weights, xform_clip, rows_per_image=None, image_sizes=None):
            return 4 * (2 * rel_codes.numel() + boxes.numel())  # deltas + boxes read, decoded boxes written

        def smooth_l1_bytes(box_regression, regression_targets, positives, labels, column0, beta, denominator, need_grad=True):
            return positives.numel() * (8 + 32) + (4 * box_regression.numel() if need_grad else 0)

        def rois_bytes(boxes, image_ids=None):
            return 36 * sum(b.shape[0] for b in boxes)

        def gather_rows_bytes(index, boxes_a=None, boxes_b=None, ints_a=None, ints_b=None):
            per_row = 8 + 32 * (boxes_a is not None) + 32 * (boxes_b is not None) + 16 * (ints_a is not None) + 16 * (ints_b is not None)
            return index.numel() * per_row

        self._wrap("box_decode", box_decode_bytes)
        self._wrap("smooth_l1_picked_fwd_bwd", smooth_l1_bytes)
        self._wrap("rois_from_boxes", rois_bytes)
        self._wrap("gather_rows", gather_rows_bytes)
        self._wrap("gemm_nt", gemm_nt_flops, "mfma_f32", gemm_nt_bytes)
        self._wrap("region_noun_align", align_bytes)
        self._wrap("weighted_ce_fwd_bwd", ce_bytes)
        self._wrap("mask_bce_stochastic_fwd_bwd", bce_bytes)
        self._wrap("split_gemm_pair", split_gemm_flops, "mfma", split_gemm_bytes, nt_shape)
        self._wrap("split_gemm_pair_gated", split_gemm_flops, "mfma", split_gemm_gated_bytes, nt_shape)
        self._wrap("split_gemm_pair_rp_gated", split_gemm_flops, "mfma", split_gemm_rp_gated_bytes, nt_shape)

        def split_gemm_pool_bytes(a_pair, b_pair, bias, residual_pair, relu, out_f32, out_pair, pool_rows):
            m, n = a_pair.shape[0], b_pair.shape[0]   # operands, the pair shortcut, whichever results are written, the pooled rows
            return (2 * a_pair.numel() + 2 * b_pair.numel() + (4 * m * n if residual_pair is not None else 0)
                    + 4 * m * n * (int(bool(out_f32)) + int(bool(out_pair))) + 4 * (m // pool_rows) * n)

        def pool_shape(a_pair, b_pair, *args, **kwargs):
            return (a_pair.shape[0], b_pair.shape[0], b_pair.shape[1] // 2, 1)

        self._wrap("split_gemm_pair_rp_pool", split_gemm_flops, "mfma", split_gemm_pool_bytes, pool_shape)
        self._wrap("split_gemm_pair_tn", split_gemm_tn_flops, "mfma", split_gemm_tn_bytes, tn_shape)

    def summary(self):
        out = {}
        for name, recs in self.records.items():
            ms = sum(r[0].elapsed_time(r[1]) for r in recs)
            work = sum(r[2] for r in recs)
            if self.kind[name] == "mfma":
                # issued = 3 bf16 hi/lo products x 2*M*N*K; algorithmic = the fp32 product the caller asked for, 2*M*N*K
                out[name] = {"launches": len(recs), "avg_us": 1e3 * ms / len(recs), "bound": "mfma",
                             "issued_GFLOP_per_launch": work / len(recs) / 1e9,
                             "alg_GFLOP_per_launch": work / 3.0 / len(recs) / 1e9,
                             "achieved_TFLOPs": work / ms / 1e9 if ms > 0 else 0.0,
                             "fp32_equiv_TFLOPs": work / 3.0 / ms / 1e9 if ms > 0 else 0.0,
                             "alg_MB_per_launch": self.bytes.get(name, 0.0) / len(recs) / 1e6}
            elif self.kind[name] == "mfma_f32":
                out[name] = {"launches": len(recs), "avg_us": 1e3 * ms / len(recs), "bound": "mfma (fp32 inputs)",
                             "alg_GFLOP_per_launch": work / len(recs) / 1e9,
                             "achieved_TFLOPs": work / ms / 1e9 if ms > 0 else 0.0,
                             "frac_of_fp32_mfma_peak": work / ms / 1e9 / MFMA_F32_PEAK_TFLOPS if ms > 0 else 0.0,
                             "alg_MB_per_launch": self.bytes.get(name, 0.0) / len(recs) / 1e6}
            else:
                out[name] = {"launches": len(recs), "avg_us": 1e3 * ms / len(recs), "bound": "hbm",
                             "alg_MB_per_launch": work / len(recs) / 1e6,
                             "achieved_GBps": work / ms / 1e6 if ms > 0 else 0.0}
        return out


def per_shape_rows(timer, steps):
    """One row per distinct (op, M, N, K, taps) of the split GEMM family: launches per step, mean microseconds, bf16
    TFLOP/s issued (6*M*N*K), fp32-equivalent TFLOP/s (2*M*N*K), 128x128 tiles and rounds of resident workgroups."""
    rows = []
    for name, recs in timer.records.items():
        if timer.kind[name] != "mfma":
            continue
        by = {}
        for r in recs:
            by.setdefault(r[3], []).append((r[0].elapsed_time(r[1]), r[2]))
        for shape, lst in by.items():
            m, n, k, taps = shape
            ms = sum(x[0] for x in lst) / len(lst)
            fl = lst[0][1]
            if name == "split_gemm_pair_tn":
                tiles, slots = (n // 128) * (k // 128), 512
            else:
                tiles = -(-m // 128) * -(-n // 128)
                slots = 1024 if (taps == 1 and tiles >= 2048) else 768 if (taps > 1 and tiles >= 1024) else 512
            rows.append((name, m, n, k, taps, len(lst) / steps, 1e3 * ms, fl / ms / 1e9, fl / 3 / ms / 1e9, tiles,
                         tiles / slots, 1e3 * ms * len(lst) / steps))
    rows.sort(key=lambda r: -r[-1])
    return rows


# bench.py op name -> kernel family of the committed PMC summary (profiles/r1_pmc_step_hbm_traffic_<workload>.json)
PMC_KERNEL = {"split_gemm_pair": "split_gemm_kernel", "split_gemm_pair_gated": "split_gemm_kernel",
              "split_gemm_pair_rp_gated": "split_gemm_kernel", "split_gemm_pair_rp_pool": "split_gemm_kernel",
              "split_gemm_pair_tn": "split_gemm_tn_kernel", "gate_split_pair": "gate_split_pair_kernel",
              "split_pair": "split_pair_kernel", "roi_align_forward_strided_pair": "roi_align_fwd_nhwc_in_strided_lds_kernel",
              "roi_align_forward_strided_nhwc": "roi_align_fwd_strided_nhwc_kernel",
              "roi_align_backward_strided": "roi_bwd_mfma_kernel", "roi_align_backward_strided_nhwc": "roi_bwd_mfma_kernel",
              "roi_align_backward": "roi_bwd_mfma_kernel"}


def _latest_profile(stem):
    """The newest round's committed summary ``profiles/r<N>_<stem>.json`` ('' when there is none)."""
    import glob
    import re
    found = []
    for q in glob.glob(os.path.join(ROOT, "profiles", f"r*_{stem}.json")):
        m = re.match(r"r(\d+)_", os.path.basename(q))
        if m:
            found.append((int(m.group(1)), q))
    return max(found)[1] if found else ""


def _stale(d, fam):
    """Why the committed summary ``d`` no longer describes kernel family ``fam`` of THIS tree (None: it does)."""
    from cvpr22_cross_modal_pseudo_labeling_amd.utils import provenance
    return provenance.stale_reason(d, fam)


def pmc_traffic(workload, op):
    """HBM bytes per launch of the dominant kernel from the rocprofv3 --pmc passes over this same step (FETCH_SIZE and
    WRITE_SIZE in separate passes, gfx950 correction applied: tools/pmc_step.sh); counters cannot be collected from
    inside the process, so the committed summary of the last pass is reported -- or null when there is none, or when the
    kernel's source has changed since that pass (the summary stamps the digests of csrc/: utils/provenance.py)."""
    path = _latest_profile(f"pmc_step_hbm_traffic_{workload}")
    fam = PMC_KERNEL.get(op)
    try:
        with open(path) as f:
            d = json.load(f)
        k = d["kernels"][fam]
    except (OSError, KeyError, ValueError):
        return None, "no PMC summary for this kernel under profiles/"
    why = _stale(d, fam)
    if why:
        return None, f"profiles/{os.path.basename(path)} is STALE for {fam}: {why}; re-collect with tools/pmc_step.sh"
    return (k["hbm_MB_per_launch"] * 1e6,
            f"bytes per launch of {fam} (all {k['launches']} launches, gated ones included): read {k['read_MB_per_launch']} MB "
            f"+ write {k['write_MB_per_launch']} MB, from profiles/{os.path.basename(path)} ({d['correction']})")


def pmc_mfma_busy(workload, op):
    """Matrix-pipe busy fraction of the dominant kernel family from hardware counters (SQ_VALU_MFMA_BUSY_CYCLES against
    the dispatch's active clocks x 1024 SIMDs = rocprofv3's MfmaUtil): the committed summary of the tools/pmc_mfma.sh pass
    over this same step (counters cannot be read from inside the process), or null."""
    path = _latest_profile(f"pmc_mfma_busy_{workload}")
    fam = PMC_KERNEL.get(op)
    try:
        with open(path) as f:
            d = json.load(f)
        frac = d["families"][fam]["mfma_busy_frac"]
    except (OSError, KeyError, ValueError):
        return None, "no MFMA-busy PMC summary for this kernel under profiles/"
    why = _stale(d, fam)
    if why:
        return None, f"profiles/{os.path.basename(path)} is STALE for {fam}: {why}; re-collect with tools/pmc_mfma.sh"
    per = {k: v["mfma_busy_frac"] for k, v in d["kernels"].items() if k.startswith(fam + "<") and "mfma_busy_frac" in v}
    return frac, (f"SQ_VALU_MFMA_BUSY_CYCLES / (1024 SIMDs x active clocks) over all launches of {fam} in the step, from "
                  f"profiles/{os.path.basename(path)}; per template instance: {per}")


def _median_ms(fn, reps=5):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    ts.sort()
    return ts[len(ts) // 2]


def reference_cpu_step_record():
    """The reference's OWN student-teacher training step timed on CPU cores -- measured in the BUILD CONTAINER (the reference
    does not travel to the GPU box) by tests/golden/time_reference_cpu_step.py and committed under profiles/: quoted here, never
    re-measured, so that the extrapolated estimate next to it can be read against a real run."""
    import re
    path = os.path.join(ROOT, "profiles", "r5_reference_cpu_step_build_container.txt")
    try:
        text = open(path).read()
        m = re.search(r"=\s*([0-9.]+) s per image = ([0-9.]+) images/s", text)
        t = re.search(r"(\d+) CPU threads", text)
        return {"value": float(m.group(2)), "unit": "images/sec", "seconds_per_image": float(m.group(1)), "cores": int(t.group(1)),
                "kind": "reference", "where": "build container, not this box", "source": "profiles/" + os.path.basename(path)}
    except (OSError, AttributeError, ValueError):
        return None


def cpu_baseline(workload):
    """The reference's own CPU kernels (oracle/_ref; the C port when it was not built) on the native-op work of the step,
    on the host cores: median of 5 per op on a bounded sample (RoIAlign is linear in the RoI count: 512 RoIs are timed and
    scaled; NMS at the step's full K), single-threaded as the reference runs them (cpu/ROIAlign_cpu.cpp:133 has its OpenMP
    pragma commented out), plus an all-cores leg (one image per thread through the bit-identical C port, whose ctypes calls
    release the interpreter lock) and a torch-CPU timing of the res5 head / trunk convolutions so that a full-step CPU
    figure exists next to the native-op one.  ~25 s of host time in total."""
    import concurrent.futures

    import torch.nn.functional as F

    import oracle

    oracle.build(with_ref=False)
    ref = oracle.ref_module()
    g = torch.Generator().manual_seed(1234)
    feat = torch.randn(1, 1024, 50, 84, generator=g)
    sample_r = 512

    def rois(r):
        xy = torch.rand(r, 2, generator=g) * torch.tensor([1066.0, 640.0])
        wh = torch.rand(r, 2, generator=g) * 300 + 16
        return torch.cat([torch.zeros(r, 1), xy, (xy + wh).clamp(max=799)], 1)

    def boxes(k):
        xy = torch.rand(k, 2, generator=g) * torch.tensor([1200.0, 720.0])
        wh = torch.rand(k, 2, generator=g) * 200 + 8
        return torch.cat([xy, xy + wh], 1), torch.rand(k, generator=g)

    if workload == "student":
        roi_counts, nms_counts = [1000, 5, 512, 512], [6000, 12000]
        res5_fwd_rois, res5_bwd_rois = 1000 + 5 + 512 + 512, 512 + 512   # per image: frozen teacher passes + student passes
    else:
        roi_counts, nms_counts = [512], [12000]
        res5_fwd_rois, res5_bwd_rois = 512, 512
    torch.set_num_threads(1)  # the reference kernels are single-threaded
    t_start = time.perf_counter()
    rr = rois(sample_r)
    roi_fn = (lambda: ref.roi_align_forward(feat, rr, 1 / 16, 14, 14, 0)) if ref is not None else \
        (lambda: oracle.roi_align_forward(feat, rr, 1 / 16, 14, 14, 0))
    per_op = {f"roi_align_forward_R{sample_r}": _median_ms(roi_fn)}
    for k in nms_counts:
        b, sc = boxes(k)
        nms_fn = (lambda: ref.nms(b, sc, 0.7)) if ref is not None else (lambda: oracle.nms(b, sc, 0.7))
        per_op[f"nms_K{k}"] = _median_ms(nms_fn)
    native_ms = sum(per_op[f"roi_align_forward_R{sample_r}"] * r / sample_r for r in roi_counts) + \
        sum(per_op[f"nms_K{k}"] for k in nms_counts)

    # all cores: one image's sample per thread through the C port (bit-identical to the reference kernels, tests/test_oracle.py)
    threads = max(1, min(os.cpu_count() or 1, 64))
    bk, sk = boxes(nms_counts[0])

    def one_image_sample(_):
        oracle.roi_align_forward(feat, rr, 1 / 16, 14, 14, 0)
        oracle.nms(bk, sk, 0.7)

    one_image_sample(0)
    t0 = time.perf_counter()
    one_image_sample(0)
    t_one = time.perf_counter() - t0
    with concurrent.futures.ThreadPoolExecutor(threads) as ex:
        t0 = time.perf_counter()
        list(ex.map(one_image_sample, range(threads)))
        t_all = time.perf_counter() - t0
    speedup = threads * t_one / t_all

    # convolutions: torch CPU (all cores), res5 head forward and forward + backward on 8 RoIs, trunk forward on one image
    torch.set_num_threads(threads)
    w1 = torch.randn(512, 1024, 1, 1) * 0.02
    w2 = torch.randn(512, 512, 3, 3) * 0.02
    w3 = torch.randn(2048, 512, 1, 1) * 0.02
    wd = torch.randn(2048, 1024, 1, 1) * 0.02
    w1b = torch.randn(512, 2048, 1, 1) * 0.02
    ws = [w1, w2, w3, wd, w1b]

    def res5(x):
        y = F.relu(F.conv2d(x, w1, stride=2))
        y = F.relu(F.conv2d(y, w2, padding=1))
        y = F.relu(F.conv2d(y, w3) + F.conv2d(x, wd, stride=2))
        for _ in range(2):
            t = F.relu(F.conv2d(y, w1b))
            t = F.relu(F.conv2d(t, w2, padding=1))
            y = F.relu(F.conv2d(t, w3) + y)
        return y

    xr = torch.randn(8, 1024, 14, 14)
    with torch.no_grad():
        per_op["res5_forward_R8_torch_cpu"] = _median_ms(lambda: res5(xr), 3)
    for w in ws:
        w.requires_grad_(True)
    per_op["res5_forward_backward_R8_torch_cpu"] = _median_ms(lambda: res5(xr).sum().backward(), 3)
    fwd_per_roi = per_op["res5_forward_R8_torch_cpu"] / 8
    fb_per_roi = per_op["res5_forward_backward_R8_torch_cpu"] / 8
    conv_ms = fwd_per_roi * (res5_fwd_rois - res5_bwd_rois) + fb_per_roi * res5_bwd_rois
    full_ms = native_ms / max(speedup, 1.0) + conv_ms  # trunk (65 GFLOP / image) not included: res5 dominates
    host_s = time.perf_counter() - t_start
    return {"value": 1e3 / native_ms, "unit": "images/sec", "cores": 1, "kind": "reference" if ref is not None else "port",
            "sample": (f"native ops of one image of the {workload} step only (RoIAlign fwd R={roi_counts} on [1,1024,50,84] -- timed "
                       f"at R={sample_r} and scaled linearly -- and NMS K={nms_counts}, thr .7), median of 5 per op, the reference's "
                       "single-threaded CPU kernels; convolutions, heads and backward excluded because the reference cannot train "
                       "on CPU (ROIAlign.h:44) -- an UPPER bound on CPU images/sec"),
            "per_op_median_ms": {k: round(v, 3) for k, v in per_op.items()},
            "all_cores": {"value": 1e3 / native_ms * speedup, "unit": "images/sec", "cores": threads, "kind": "port",
                          "sample": f"{threads} threads, one image sample (RoIAlign R={sample_r} + NMS K={nms_counts[0]}) each through "
                                    f"the C port; measured speed-up x{speedup:.1f} applied to the single-thread figure"},
            "reference_own_step": reference_cpu_step_record(),
            "full_step_estimate": {"value": 1e3 / full_ms, "unit": "images/sec", "cores": threads,
                                   "method": (f"native ops on all cores + torch-CPU res5 head on all cores: {res5_fwd_rois} RoIs forward of "
                                              f"which {res5_bwd_rois} also backward per image ({fwd_per_roi:.1f} / {fb_per_roi:.1f} ms per RoI); "
                                              "trunk and heads not included -- still an upper bound")},
            "host_cpus": os.cpu_count(), "host_seconds": round(host_s, 1)}


GRAD_SAMPLE_PER_PARAM = 4096
DUMP_LIMIT_BYTES = 64 << 20


def last_step_outputs(loss_dict, model):
    """What a caller of the timed step holds after its last call, as host arrays: every loss term the step returned
    (float64, named after the term) and ``grad_sample`` -- up to GRAD_SAMPLE_PER_PARAM entries of every trainable
    parameter's gradient in ``named_parameters`` order, at indices drawn from a fixed seed (float32; all gradients would
    be several times the 64 MB the dump may take)."""
    import re
    out = {re.sub(r"[^\w.-]", "_", k): v.detach().double().cpu().numpy() for k, v in loss_dict.items()}
    g = torch.Generator().manual_seed(4321)
    parts = []
    for _, p in model.named_parameters():
        if not p.requires_grad or p.grad is None:
            continue
        flat = p.grad.detach().reshape(-1)
        if flat.numel() > GRAD_SAMPLE_PER_PARAM:
            idx = torch.randint(0, flat.numel(), (GRAD_SAMPLE_PER_PARAM,), generator=g).sort().values
            flat = flat[idx.to(flat.device)]
        parts.append(flat.float().cpu())
    out["grad_sample"] = (torch.cat(parts) if parts else torch.zeros(0)).numpy()
    return out


def write_outputs(outputs, path):
    import numpy as np
    total = sum(a.nbytes for a in outputs.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit(f"bench.py --dump-outputs: {total} bytes exceed the {DUMP_LIMIT_BYTES}-byte limit")
    os.makedirs(path, exist_ok=True)
    for name, a in outputs.items():
        np.save(os.path.join(path, name + ".npy"), a)


TINY_OVERRIDES = ["MODEL.RPN.PRE_NMS_TOP_N_TRAIN", 300, "MODEL.RPN.PRE_NMS_TOP_N_TEST", 200, "MODEL.RPN.POST_NMS_TOP_N_TRAIN", 60,
                  "MODEL.RPN.POST_NMS_TOP_N_TEST", 40, "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", 16]
TINY_BATCH = dict(height=128, width=160, num_gt=3, num_nouns=2, n_vocab=50)


def roi_align_micro(dev, iters=200, warm_seconds=0.3):
    """RoIAlign on the shape the north_star's `ROIAlign-bwd >= 60 % of HBM` target is quoted on (R = 1024 RoIs,
    C = 1024, 2 x 50 x 84 map, 14 x 14 bins, fp32 NCHW both sides: 856.5 MB algorithmic = grad_output / output once + the
    map once), through the reference operator API (`_C.roi_align_backward` / `_C.roi_align_forward`).  HIP events on the
    launch stream over `iters` launches after `warm_seconds` of the same op; plan + main kernel of the backward both inside.
    One second of wall time; goes into `config` so the driver's record carries it."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    n, c, h, w, r = 2, 1024, 50, 84, 1024
    g = torch.Generator().manual_seed(1234)
    alg = 4 * r * c * 196 + 4 * n * c * h * w + 20 * r
    out = {"shape": f"R={r} C={c} map {n}x{h}x{w} bins 14x14 fp32", "alg_MB": round(alg / 1e6, 1), "iters": iters}

    def rois(kind):
        b = torch.randint(0, n, (r, 1), generator=g).float()
        if kind == "uniform":  # x1 ~ U[0,1066], y1 ~ U[0,640], w, h ~ U[16,316], clipped
            x1, y1 = torch.rand(r, 1, generator=g) * 1066, torch.rand(r, 1, generator=g) * 640
            ww, hh = torch.rand(r, 1, generator=g) * 300 + 16, torch.rand(r, 1, generator=g) * 300 + 16
        else:  # RPN-like: log-uniform areas 32^2 .. 512^2, aspect ratios {.5, 1, 2}
            area = torch.exp(torch.rand(r, 1, generator=g) * (2 * math.log(512.0 / 32)) + 2 * math.log(32.0))
            ratio = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (r, 1), generator=g)]
            ww, hh = torch.sqrt(area / ratio), torch.sqrt(area * ratio)
            x1, y1 = torch.rand(r, 1, generator=g) * (1333 - ww).clamp(min=1), torch.rand(r, 1, generator=g) * (800 - hh).clamp(min=1)
        return torch.cat([b, x1, y1, (x1 + ww).clamp(max=1332), (y1 + hh).clamp(max=799)], 1).to(dev)

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < warm_seconds:
            for _ in range(10):
                fn()
            torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        us = 1e3 * a.elapsed_time(b) / iters
        return {"us": round(us, 1), "frac_hbm": round(alg / us / 1e3 / HBM_PEAK_GBS, 4)}

    x = torch.randn(n, c, h, w, generator=g).to(dev)
    go = torch.randn(r, c, 14, 14, generator=g).to(dev)
    for kind in ("uniform", "rpn_like"):
        rr = rois(kind)
        out[f"backward_{kind}"] = timed(lambda: _C.roi_align_backward(go, rr, 1 / 16, 14, 14, n, c, h, w, 0))
        out[f"forward_{kind}"] = timed(lambda: _C.roi_align_forward(x, rr, 1 / 16, 14, 14, 0))
    return out


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=None,
                    help="ranks of the job (default: WORLD_SIZE under a launcher, else 1); N > 1 without a launcher environment "
                         "makes this process the launcher of its N ranks")
    ap.add_argument("--steps", type=int, default=60,
                    help="timed steps (default 60 = 2 s of student steps: a region long enough that the box-to-box spread, not its own noise, bounds the line)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="student", choices=["student", "teacher"])
    ap.add_argument("--contention-copy-mb", type=float, default=0.0,
                    help="per step, device-to-device copies of this many MB in three pieces on a separate stream (an upper bound "
                         "on what an N-GPU job's gradient exchange costs the backward it overlaps; see Feed.add_contention)")
    ap.add_argument("--full", action="store_true",
                    help="beyond the headline: sequential replay with per-kernel / roofline figures, the secondary (teacher) "
                         "region, the RoIAlign micro-benchmark and the CPU baseline (the --no-* switches below thin it out)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy: every loss term "
                         "(float64) and grad_sample (float32: a seeded sample of every trainable parameter's gradient)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roi-micro", action="store_true",
                    help="skip the one-second RoIAlign micro-benchmark (config.roi_align_backward_856MB) after the steps")
    ap.add_argument("--min-seconds", type=float, default=0.0,
                    help="extend the timed region to at least this long (steps are added; the JSON reports the count)")
    ap.add_argument("--burn-seconds", type=float, default=3.0, help="GPU clock warm-up before the warm-up steps")
    ap.add_argument("--no-pipeline", action="store_true", help="plain sequential step (no side-stream overlap)")
    ap.add_argument("--per-shape-csv", default="", help="write one row per distinct split-GEMM shape of the step (needs --full)")
    ap.add_argument("--secondary-steps", type=int, default=10,
                    help="with --full, after the student region: this many timed steps of the teacher configuration "
                         "(zeroshot_mask.yaml, BASELINE config 2) reported under `secondary`; 0 = skip")
    # DRY RUN of the multi-rank control flow without GPUs: the same rank code (rendezvous, parameter broadcast, barriers,
    # step-count calibration, MAX-reduce of the elapsed time, replay on every rank with live all-reduces, per-rank gather)
    # on the product's own host path (MODEL.DEVICE cpu, BASELINE configs[0]) over gloo.  Never a measurement.
    ap.add_argument("--device", default="cuda", choices=["cuda", "cpu"], help="cpu = DRY RUN on the in-package host path")
    ap.add_argument("--backend", default=None, help="torch.distributed backend (default: nccl = RCCL on cuda, gloo on cpu)")
    ap.add_argument("--tiny", action="store_true", help="DRY RUN size: 128x160 images, a few dozen RoIs")
    ap.add_argument("--share-gpu", action="store_true",
                    help="DRY RUN on a box with fewer GPUs than ranks: rank r runs on device r %% visible devices (RCCL refuses two "
                         "ranks on one device, so this needs --backend gloo); exercises the DEVICE side of the N > 1 path -- "
                         "streams, hooks, the pipelined trainer next to live collectives -- never a measurement")
    ap.add_argument("--resident-input", action="store_true",
                    help="A/B: every step re-uses ONE device-resident batch (no host-to-device staging in the timed region)")
    ap.add_argument("--host-batches", type=int, default=4, help="distinct pinned host batches the staged input stream cycles through")
    ap.add_argument("--fault-inject", default="", help=argparse.SUPPRESS)  # "RANK:STEP": that rank dies inside the timed region (tests)
    args = ap.parse_args(argv)
    if args.per_shape_csv and not args.full:
        ap.error("--per-shape-csv comes from the sequential replay of --full")
    return args


class Feed:
    """The step's input stream.  Staged (default): ``--host-batches`` distinct synthetic batches live in PINNED host memory;
    a ``DevicePrefetcher`` thread copies one per step to the device on its own stream, two steps ahead (images 25.6 MB +
    ground-truth masks 15 MB per step at 2 x 3 x 800 x 1333) -- what engine/trainer.py:103-107 of the reference does inside
    its loop, off the training thread.  Resident (``--resident-input``): the same device batch every step."""

    def __init__(self, args, dev, rank, batch_kw, warmup):
        from cvpr22_cross_modal_pseudo_labeling_amd.data.prefetch import DevicePrefetcher, _map
        from cvpr22_cross_modal_pseudo_labeling_amd.data.synthetic import make_batch
        self.staged = not args.resident_input
        self.prefetcher = None
        if not self.staged:
            self.cur = self.nxt = make_batch(IMS_PER_GPU, device=dev, seed=1234 + rank, **batch_kw)
            self.first_images = self.cur[0]
            return
        pin = (lambda t: t.pin_memory()) if dev.type == "cuda" else (lambda t: t)
        # every distinct batch passes through the warm-up steps once (its RoI counts size the caching allocator's blocks:
        # a batch first seen inside the timed region costs hipMallocs there -- 31 vs 22.5 ms per teacher step over 10 steps)
        n_pool = max(1, min(args.host_batches, warmup - 1))
        pool = [_map(make_batch(IMS_PER_GPU, device="cpu", seed=1234 + rank + 1000 * i, **batch_kw), pin)
                for i in range(n_pool)]
        self.pool_size = n_pool
        self.bytes_per_step = sum(t.numel() * t.element_size() for b in pool[:1] for t in self._tensors(b))

        def cycle():
            i = 0
            while True:
                yield pool[i % len(pool)]
                i += 1

        self.prefetcher = DevicePrefetcher(cycle(), dev, depth=2)
        self.cur, self.nxt = next(self.prefetcher), next(self.prefetcher)
        self.first_images = self.cur[0]

    @staticmethod
    def _tensors(obj):
        if torch.is_tensor(obj):
            yield obj
        elif isinstance(obj, (list, tuple)):
            for o in obj:
                yield from Feed._tensors(o)
        elif hasattr(obj, "bbox"):
            yield obj.bbox
            for v in obj.extra_fields.values():
                yield from Feed._tensors(v)

    def add_contention(self, dev, mbytes, pieces=3):
        """--contention-copy-mb: beside every step, `pieces` device-to-device copies of mbytes / pieces each on a stream of
        their own -- what the gradient exchange of an N-GPU job adds to this GPU while the backward runs (RCCL's kernels read
        and write the buckets: ~2 x payload of HBM traffic and a few workgroups), with no second GPU at hand.  The step-time
        delta against a run without it bounds the contention term of the 1 -> N curve from above (the copies are not
        throttled by a wire)."""
        n = max(1, int(mbytes * 1e6 / 4 / pieces))
        self._cont = [(torch.empty(n, device=dev), torch.empty(n, device=dev)) for _ in range(pieces)]
        self._cont_stream = torch.cuda.Stream(device=dev)
        self.contention_mb = pieces * n * 4 / 1e6

    def step(self, pipe):
        """One optimisation step on the current batch with the next one as look-ahead, then advance."""
        (images, targets), nxt = self.cur, self.nxt
        if getattr(self, "_cont", None):
            with torch.cuda.stream(self._cont_stream):
                for src, dst in self._cont:
                    dst.copy_(src, non_blocking=True)
        out = pipe.step(images, targets, nxt)
        if self.staged:
            self.cur, self.nxt = nxt, next(self.prefetcher)
        return out

    def close(self):
        if self.prefetcher is not None:
            self.prefetcher.close()


def build_workload(args, workload, dev, world, rank, warmup):
    from cvpr22_cross_modal_pseudo_labeling_amd.config import get_defaults
    from cvpr22_cross_modal_pseudo_labeling_amd.data.synthetic import calibrate_stem_bn, make_embeddings
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import comm, solver, trainer
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.detector import build_detection_model

    cfg = get_defaults()
    name = "student_teacher_mask_rcnn_uncertainty" if workload == "student" else "zeroshot_mask"
    cfg.merge_from_file(os.path.join(ROOT, "configs", "coco_cap_det", name + ".yaml"))
    # synthetic run: a tiny LR keeps random-init weights finite over many steps (the optimizer step still runs)
    cfg.merge_from_list(["SOLVER.BASE_LR", 1e-6, "SOLVER.IMS_PER_BATCH", IMS_PER_GPU * world, "MODEL.DEVICE", dev.type]
                        + (TINY_OVERRIDES if args.tiny else []))
    cfg.freeze()
    torch.manual_seed(1234)  # identical initial weights on every rank; broadcast anyway
    model = build_detection_model(cfg).to(dev)
    batch_kw = TINY_BATCH if args.tiny else {}
    e_vocab, e_seen = make_embeddings(cfg.MODEL.ROI_BOX_HEAD.EMB_DIM, seed=1234, device=dev,
                                      **({"n_vocab": TINY_BATCH["n_vocab"]} if args.tiny else {}))
    model.set_class_embeddings(e_seen)
    if hasattr(model, "set_caption_vocab"):
        model.set_caption_vocab(e_vocab)
    feed = Feed(args, dev, rank, batch_kw, warmup)
    if args.contention_copy_mb > 0 and dev.type == "cuda":
        feed.add_contention(dev, args.contention_copy_mb)
    calibrate_stem_bn(model, feed.first_images)
    comm.broadcast_parameters(model)
    model.train()
    optimizer = solver.make_optimizer(cfg, model)
    scheduler = solver.make_lr_scheduler(cfg, optimizer)
    reducer = comm.BucketedGradReducer(model)
    reducer.measure_wait = world > 1
    pipe = trainer.PipelinedTrainer(model, optimizer, reducer, scheduler)
    if args.no_pipeline:
        pipe.enabled = False
    return name, model, feed, reducer, pipe


def run_secondary(args, dev, world, rank, on_gpu, timer, sync):
    """A short timed region of the teacher configuration (zeroshot_mask.yaml, BASELINE config 2) after the student one: same
    protocol (warm-up, barrier + synchronize on both sides, MAX over ranks).  Returns the `secondary` object (rank 0) or None."""
    secondary = None
    warm2 = 8  # the student model was just released and the allocator emptied: a few more steps than the pool of distinct batches
    name2, model2, feed2, reducer2, pipe2 = build_workload(args, "teacher", dev, world, rank, warm2)
    # (the teacher step runs its frozen trunk prefix -- stem + layer1 -- of the next batch ahead)
    for _ in range(warm2):
        feed2.step(pipe2)
    sync()
    overlapped2 = pipe2.enabled
    timer.enabled = on_gpu and not overlapped2
    t0 = time.perf_counter()
    marks2 = []
    for _ in range(args.secondary_steps):
        loss2 = feed2.step(pipe2)
        marks2.append(time.perf_counter())
    sync()
    el2 = time.perf_counter() - t0
    timer.enabled = False
    pipe2.drain()
    replay2 = 0
    if overlapped2 and on_gpu:  # per-kernel figures from a sequential replay, as for the primary workload
        replay2 = 3
        pipe2.enabled = False
        for _ in range(2):
            feed2.step(pipe2)
        sync()
        timer.enabled = True
        for _ in range(replay2):
            feed2.step(pipe2)
        sync()
        timer.enabled = False
    if world > 1:
        t = torch.tensor([el2], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el2 = float(t.item())
    if rank == 0:
        k2 = timer.summary()
        secondary = {"workload": (f"{name2}.yaml R-50-C4 teacher, {IMS_PER_GPU} img/GPU "
                                  f"{'3x128x160 TINY' if args.tiny else '3x800x1333'}, fwd+bwd+allreduce+SGD"),
                     "steps": args.secondary_steps, "warmup": warm2, "pipelined": overlapped2, "replay_steps": replay2,
                     "ms_per_step": round(1e3 * el2 / args.secondary_steps, 3),
                     "host_issue_ms": [round(1e3 * (b - a), 2) for a, b in zip([t0] + marks2[:-1], marks2)],
                     "images_per_s": round(IMS_PER_GPU * world * args.secondary_steps / el2, 3),
                     "losses_finite": all(bool(torch.isfinite(v).all()) for v in loss2.values()),
                     "allreduce_payload_MB": round(sum(f.numel() * f.element_size() for f in reducer2.flat) / 1e6, 1),
                     "kernels": {n: {kk: round(vv, 3) if isinstance(vv, float) else vv for kk, vv in k2[n].items()}
                                 for n in ("roi_align_backward_strided", "roi_align_backward_strided_nhwc", "roi_align_forward_strided_nhwc", "split_gemm_pair",
                                           "split_gemm_pair_gated", "split_gemm_pair_tn", "nms_presorted_batched") if n in k2}}
    feed2.close()
    del pipe2, reducer2, model2, feed2
    return secondary


def main():
    args = parse_args()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus is None:
        args.gpus = world  # under a launcher (torchrun --nproc-per-node N bench.py) the flag may be omitted
    if args.gpus != world:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher environment says WORLD_SIZE={world}")
    on_gpu = args.device == "cuda"
    dry_run = (not on_gpu) or args.tiny or args.share_gpu
    if args.share_gpu and (args.backend or "nccl") == "nccl":
        raise SystemExit("bench.py --share-gpu: RCCL does not place two ranks on one device; pass --backend gloo")
    if on_gpu:
        # counting devices does not initialise the GPU.  A launcher that exports LOCAL_WORLD_SIZE tells how many ranks share
        # this node; without it (older launchers, multi-node) only this rank's own device index can be checked.
        need = 1 if args.share_gpu else int(os.environ["LOCAL_WORLD_SIZE"]) if "LOCAL_WORLD_SIZE" in os.environ else local_rank + 1
        if torch.cuda.device_count() < need:
            raise SystemExit(f"bench.py --gpus {args.gpus}: only {torch.cuda.device_count()} GPU(s) visible on this node")
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs an MI355X: the product path has no CPU fallback (--device cpu is the dry run "
                             "of the multi-rank control flow on the CPU-only configuration, not a fallback)")
        index = local_rank % torch.cuda.device_count() if args.share_gpu else local_rank
        torch.cuda.set_device(index)
        if "OMP_NUM_THREADS" not in os.environ:
            # the GPU path does almost no CPU math, but a machine-wide OpenMP team spinning behind every small host op starves
            # the staging thread / loader workers (tools/train_net.py); the CPU-baseline leg sets its own thread counts
            torch.set_num_threads(max(1, min(8, len(os.sched_getaffinity(0)) // 4)))
        dev = torch.device("cuda", index)
    else:
        dev = torch.device("cpu")
        torch.set_num_threads(max(1, int(os.environ.get("OMP_NUM_THREADS", "2"))))
    backend = args.backend or ("nccl" if on_gpu else "gloo")
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if on_gpu and backend == "nccl":
            dist.init_process_group(backend, init_method="env://", device_id=dev)
        else:
            dist.init_process_group(backend, init_method="env://")
    fault = tuple(int(x) for x in args.fault_inject.split(":")) if args.fault_inject else None

    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    name, model, feed, reducer, pipe = build_workload(args, args.workload, dev, world, rank, args.warmup)
    timer = OpTimer(_C)
    if on_gpu and args.full:
        timer.install()

    def sync():
        if world > 1:
            dist.barrier()
        if on_gpu:
            torch.cuda.synchronize()

    # Student-teacher workload: two-stream software pipeline (engine/trainer.py::PipelinedTrainer) -- the frozen half
    # (trunk, RPN, teacher pseudo-labelling) of step k+1 overlaps the student backward of step k.  Every timed step
    # still executes one frozen half and one student half on a batch the staging thread copied in from pinned host memory
    # (Feed: a different one of --host-batches synthetic batches per step; --resident-input = one device batch throughout).
    # Device warm-up (not a training step): a fresh, idle GPU takes a few seconds of load to reach its sustained clocks,
    # and the first process on a box measured 12-20 % slower without it.
    if on_gpu and args.burn_seconds > 0:
        burn = torch.randn(8192, 8192, device=dev, dtype=torch.bfloat16)
        t_burn = time.perf_counter()
        while time.perf_counter() - t_burn < args.burn_seconds:
            for _ in range(20):
                burn @ burn
            torch.cuda.synchronize()
        del burn
    for _ in range(args.warmup):
        feed.step(pipe)
    sync()
    overlapped = pipe.enabled
    # sequential workloads under --full: per-kernel HIP-event timing live in the timed region
    timer.enabled = on_gpu and args.full and not overlapped
    if args.min_seconds > 0:  # calibrate the step count on a short untimed probe (same count on every rank)
        t0 = time.perf_counter()
        for _ in range(3):
            feed.step(pipe)
        sync()
        probe = torch.tensor([(time.perf_counter() - t0) / 3], device=dev, dtype=torch.float64)
        if world > 1:
            dist.all_reduce(probe, op=dist.ReduceOp.MAX)
        args.steps = max(args.steps, int(args.min_seconds / float(probe.item())) + 1)
        timer.records.clear()
    reducer.exposed_wait_ms()  # drop the warm-up / probe records
    # the K timed steps, bracketed by barrier + synchronize; in between, un-synchronised host timestamps every few
    # steps give the spread of the step time inside the region (they do not stall the pipeline)
    chunk = max(1, args.steps // 8)
    marks = []
    t0 = time.perf_counter()
    for i in range(args.steps):
        if fault is not None and fault == (rank, i):
            os._exit(13)  # test hook: a rank lost inside the timed region must end the whole job with a non-zero code
        loss_dict = feed.step(pipe)
        if (i + 1) % chunk == 0:
            marks.append((i + 1, time.perf_counter()))
    sync()
    own_elapsed = elapsed = time.perf_counter() - t0
    chunk_ms = [1e3 * (b[1] - a[1]) / (b[0] - a[0]) for a, b in zip(marks[:-1], marks[1:])]
    pipe.drain()
    if args.dump_outputs and rank == 0:
        write_outputs(last_step_outputs(loss_dict, model), args.dump_outputs)
    waits = reducer.exposed_wait_ms()
    hook_launches, n_buckets = reducer.hook_launches, len(reducer.buckets)
    timer.enabled = False
    replay_steps = 0
    if args.full and (overlapped or not on_gpu):
        # In the pipelined step two streams share the GPU, so an event pair around one kernel also spans kernels of the
        # other stream.  The per-kernel roofline figures therefore come from a sequential replay of the same step
        # right after the timed region (same launches, one stream); `value` is the pipelined, timed region only.
        # (The dry run has nothing to time per kernel; it replays so that this branch -- every rank, live all-reduces --
        # has executed somewhere before an 8-GPU node sees it.)
        replay_steps = max(3, args.steps // 4)
        pipe.enabled = False
        for _ in range(2):  # settle the caching allocator on the single-stream allocation pattern first
            feed.step(pipe)
        sync()
        timer.enabled = on_gpu
        for _ in range(replay_steps):
            feed.step(pipe)
        sync()
        timer.enabled = False
    timer.enabled = False
    per_rank = None
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        # every rank's own view of the region: its wall time, its step count, how long its finish() stalled on the
        # collectives per step (the exposed part of the exchange) and how many buckets its backward hooks issued
        gdev = dev if backend == "nccl" else torch.device("cpu")  # (gloo gathers host tensors only)
        mine = torch.tensor([own_elapsed, float(args.steps), sum(waits) / max(len(waits), 1), max(waits, default=0.0),
                             float(hook_launches)], device=gdev, dtype=torch.float64)
        gathered = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(gathered, mine)
        placed = [None] * world  # where every rank pinned itself (engine/launch.py::apply_rank_affinity)
        dist.all_gather_object(placed, AFFINITY)
        per_rank = [{"rank": r, "elapsed_s": round(float(g[0]), 4), "steps": int(g[1]),
                     "allreduce_exposed_wait_ms_mean": round(float(g[2]), 3), "allreduce_exposed_wait_ms_max": round(float(g[3]), 3),
                     "issued_from_backward_hooks": int(g[4]), "cpus": placed[r]["cpus"], "cpus_from": placed[r]["source"]}
                    for r, g in enumerate(gathered)]
    finite = all(bool(torch.isfinite(v).all()) for v in loss_dict.values())
    payload_mb = round(sum(f.numel() * f.element_size() for f in reducer.flat) / 1e6, 1)

    # Secondary figure (BASELINE config 2): a short timed region of the teacher configuration after the student one, so
    # that the driver's single command also observes the teacher step.  Same protocol (warm-up, barrier + synchronize on
    # both sides, MAX over ranks); the student model is released first.
    secondary = None
    shape_rows = per_shape_rows(timer, replay_steps or args.steps) if (args.per_shape_csv and rank == 0) else None
    if args.full and args.workload == "student" and args.secondary_steps > 0:
        kernels_primary = timer.summary() if rank == 0 else None
        timer.records.clear()
        for k in timer.bytes:
            timer.bytes[k] = 0.0
        staged, bytes_per_step, pool_size = feed.staged, getattr(feed, "bytes_per_step", 0), getattr(feed, "pool_size", 0)
        feed.close()
        del pipe, reducer, model, feed
        if on_gpu:
            torch.cuda.empty_cache()
        try:  # the headline above is complete: a failure in here must not take the line with it
            secondary = run_secondary(args, dev, world, rank, on_gpu, timer, sync)
        except Exception as e:  # noqa: BLE001 -- reported in the line
            if world > 1:
                raise  # a rank that fell out of the collectives' order cannot carry on
            secondary = {"error": f"{type(e).__name__}: {e}"[:400]}
    else:
        kernels_primary = timer.summary() if rank == 0 else None
        staged, bytes_per_step, pool_size = feed.staged, getattr(feed, "bytes_per_step", 0), getattr(feed, "pool_size", 0)
        feed.close()

    if rank == 0:
        kernels = kernels_primary
        # the roofline object describes the hand-written kernel the step spends most time in (the split GEMM:
        # matrix-core bound; the byte kernels: HBM-bound); every native op is listed under "kernels"
        dom = max(kernels, key=lambda n: kernels[n]["launches"] * kernels[n]["avg_us"]) if kernels else "none"
        k = kernels.get(dom, {"bound": "hbm", "achieved_GBps": 0.0})
        measured_in = (f"{replay_steps} sequential replay steps after the timed region (the timed steps overlap two "
                       "streams)") if replay_steps else "the timed region"
        traffic, traffic_note = pmc_traffic(args.workload, dom) if kernels else (None, None)
        mfma_busy, mfma_busy_note = pmc_mfma_busy(args.workload, dom) if kernels else (None, None)
        if not kernels:
            roofline = None  # no --full, or a dry run on the host path: no kernel was timed
        elif k["bound"] == "mfma":
            roofline = {"bound": "mfma", "kernel": dom, "achieved": k["achieved_TFLOPs"], "peak": MFMA_BF16_PEAK_TFLOPS,
                        "unit": "TFLOP/s", "frac": k["achieved_TFLOPs"] / MFMA_BF16_PEAK_TFLOPS,
                        # ALGORITHMIC flops of the fp32 convolutions (2*M*N*K) over the same time: against the bf16 matrix
                        # peak the kernel runs on, and against the fp32 matrix peak an fp32-input kernel would be priced at
                        "achieved_algorithmic": k["fp32_equiv_TFLOPs"],
                        "frac_algorithmic": k["fp32_equiv_TFLOPs"] / MFMA_BF16_PEAK_TFLOPS,
                        "frac_algorithmic_of_fp32_mfma_peak": k["fp32_equiv_TFLOPs"] / MFMA_F32_PEAK_TFLOPS,
                        "traffic": traffic,
                        "traffic_note": traffic_note,
                        "mfma_busy_frac": mfma_busy,
                        "mfma_busy_note": mfma_busy_note,
                        "note": ("bf16 matrix-core flops issued: 3 hi/lo products x 2*M*N*K per fp32-accurate product "
                                 f"({k['fp32_equiv_TFLOPs']:.0f} TFLOP/s fp32-equivalent); `peak` is the dense spec figure -- "
                                 f"the MFMA-only ablation of this loop sustains {MFMA_SUSTAINED_TFLOPS:.0f} TFLOP/s on random "
                                 "operands (DESIGN.md section 4), of which this is "
                                 f"{k['achieved_TFLOPs'] / MFMA_SUSTAINED_TFLOPS:.2f}"),
                        "measured_in": measured_in}
        else:
            roofline = {"bound": "hbm", "kernel": dom, "achieved": k["achieved_GBps"], "peak": HBM_PEAK_GBS,
                        "unit": "GB/s", "frac": k["achieved_GBps"] / HBM_PEAK_GBS, "traffic": traffic,
                        "traffic_note": traffic_note,
                        "measured_in": measured_in}
        global_batch = IMS_PER_GPU * world
        metric = ("images/sec student-teacher train step (COCO 800x1333)" if args.workload == "student"
                  else "images/sec teacher train step (COCO 800x1333)")
        size = "3x128x160 TINY" if args.tiny else "3x800x1333"
        out = {
            "metric": metric + (" [DRY RUN: control-flow check of the multi-rank path, NOT a measurement]" if dry_run else ""),
            "value": global_batch * args.steps / elapsed,
            "unit": "images/sec",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32 (bf16x3 split MFMA, fp32 accum)" if on_gpu else "f32 (host path)",
            "data": "synthetic",
            "dry_run": dry_run,
            "device": args.device,
            "backend": backend if world > 1 else None,
            # ranks whose gradients went through RCCL: 0 unless the group's backend is nccl (a one-rank job has no exchange;
            # the gloo dry runs are not RCCL)
            "rccl_ranks": dist.get_world_size() if (world > 1 and dist.is_initialized() and backend == "nccl") else 0,
            "cpus": AFFINITY,
            # gradient exchange of the last timed step: buckets whose all-reduce was issued from a backward hook (i.e.
            # overlapped with the rest of the backward) out of all buckets, the payload, and -- per step -- how long
            # finish() stalled on the collectives after the backward (max over ranks of each rank's mean)
            "allreduce": {"buckets": n_buckets, "issued_from_backward_hooks": hook_launches,
                          "payload_MB": payload_mb,
                          "op": ("AVG in the collective" if backend == "nccl" else "SUM, divided after the wait") if world > 1 else "none (1 rank)",
                          "exposed_wait_ms_per_step": (max(r["allreduce_exposed_wait_ms_mean"] for r in per_rank) if per_rank else 0.0)},
            "ranks": per_rank,
            "config": {"workload": f"{name}.yaml R-50-C4, {IMS_PER_GPU} img/GPU {size}, fwd+bwd+allreduce+SGD",
                       "global_batch": global_batch, "parallelism": f"dp{world}", "losses_finite": finite,
                       "pipelined": bool(overlapped),
                       # input staging inside the timed region (reference engine/trainer.py:103-107): pinned host batch ->
                       # device on the copy stream, every step
                       "h2d_in_timed_region": bool(staged), "h2d_MB_per_step": round(bytes_per_step / 1e6, 1),
                       "distinct_host_batches": pool_size,
                       "contention_copy_MB_per_step": args.contention_copy_mb or None,
                       # BASELINE config 2 (teacher, zeroshot_mask.yaml): same protocol, after the student region
                       "secondary_workload": (secondary or {}).get("workload"),
                       "secondary_ms_per_step": (secondary or {}).get("ms_per_step"),
                       "secondary_images_per_s": (secondary or {}).get("images_per_s")},
            # host-side step time over chunks of the timed region (issue rate of rank 0; the region total is `ms_per_step`)
            "ms_per_step_spread": ({"chunk_steps": chunk, "min": round(min(chunk_ms), 3), "median": round(sorted(chunk_ms)[len(chunk_ms) // 2], 3),
                                    "max": round(max(chunk_ms), 3)} if chunk_ms else None),
            "replay_steps": replay_steps,
            "roofline": roofline,
            "secondary": secondary,
            "kernels": {n: {kk: round(vv, 3) if isinstance(vv, float) else vv for kk, vv in v.items()}
                        for n, v in kernels.items()},
        }
        if args.per_shape_csv:
            with open(args.per_shape_csv, "w") as f:
                f.write("op,M,N,K,taps,launches_per_step,avg_us,bf16_TFLOPs_issued,fp32_equiv_TFLOPs,tiles_or_tn_tiles,"
                        "rounds_of_resident_workgroups,us_per_step\n")
                for r in shape_rows:
                    f.write(",".join(str(round(x, 3)) if isinstance(x, float) else str(x) for x in r) + "\n")
        if args.full and world == 1 and on_gpu and not args.tiny and not args.no_roi_micro:
            # the a2 target's own micro-benchmark, recorded where the driver keeps it (VERDICT r5 missing-4)
            try:
                torch.cuda.empty_cache()
                micro = roi_align_micro(dev)
                out["config"]["roi_align_backward_856MB"] = dict(micro["backward_uniform"], rois="uniform (SURVEY 8(d))")
                out["config"]["roi_align_856MB"] = micro
            except Exception as e:  # noqa: BLE001 -- the headline is complete: report, do not lose the line
                out["config"]["roi_align_backward_856MB"] = {"error": f"{type(e).__name__}: {e}"[:300]}
        if args.full and world == 1 and not args.no_cpu_baseline and on_gpu:
            out["cpu_baseline"] = cpu_baseline(args.workload)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
