"""bench.py — headline benchmark: audio-seconds/s of the wavlm-large-s80 pipeline (segmentation + embedding + AHC).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--precision f32h|f32s|f32|f16] [--minutes 30] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run sets up, warms up, times the K steps, writes --dump-outputs and prints the result line: `value`, `ms_per_step`,
`device_value`, `step_breakdown`, the per-kernel `roofline` / `kernels` that the in-situ profiler records inside those steps and
the board `power` sampled while they run.  `--full` adds every leg that takes runs of its own (`extra_legs`): the serial steps,
the other arithmetic modes, two streams, `e2e`, the strong-scaling leg, `config1` and `cpu_baseline`; their `--no-*` flags trim
a `--full` run.

`--gpus N` with N > 1 and no launcher in the environment (WORLD_SIZE unset) makes bench.py launch its own N ranks
(`torch.distributed.run --standalone`-style rendezvous on 127.0.0.1, one GPU each, RCCL); it refuses to run — non-zero
exit, clear message — when fewer than N devices are visible or when the process group that comes up does not have N
ranks.  `DZN_BENCH_ONE_DEVICE=1` (rehearsal on a 1-GPU box) maps every rank to device 0 and stages the collective
through gloo, because RCCL refuses duplicate devices.

One "step" (r5) = the WHOLE pipeline BASELINE.json configs[2] names over ONE synthetic recording per rank
(wavlm-large-s80, 30 min of 16 kHz mono, window 8 s, step 0.8 s -> 2241 windows in 4 balanced launches of 561 (--batch 576
is the maximum): windows are independent, results do not depend on the batch), the recording already resident in HBM:
for every batch of windows  segmentation (WavLM + Conformer + powerset) -> median filter + overlap-excluded masks ->
ResNet34 embeddings (trunk shared by the 4 local speakers), all through the C ABI of libdzn_hip.so; u8 decisions + f32
embeddings copied to the host (and all-gathered over RCCL at N > 1); then the HOST stage — speaker counting, centroid-linkage
AHC, constrained assignment, reconstruction, Binarize, RTTM text (diarizen/pipelines/inference.py:137-185) — through the
product's run_host_stage.  Consecutive steps are a two-stage software pipeline, as DiariZenPipeline.diarize_many runs a corpus: the
host stage of step i executes in a worker thread (own HIP stream / arena) beside the device stage of step i+1, and every step's host
stage completes inside the timed region (`--no-overlap`, `serial_value`: the serial steps).  `value` = audio of all ranks /
max-over-ranks time of the K steps; `device_value` = the device hot
path of the same steps alone (what r1-r4 called `value`); `e2e` = the same pipeline through the DiariZenPipeline object incl.
the host -> HBM upload of the recording.

Prints ONE JSON line on rank 0 (contract in the task statement) with `roofline` (in-situ HIP-event
timing of the dominant kernel class over the timed steps), `parity` (what holds the path to the reference) and, with --full,
`cpu_baseline` (the oracle — a CPU port of the reference arithmetic — on a bounded sample of the same workload), the same
workload in the other arithmetic modes, `e2e` (the whole pipeline incl. host clustering) and, with N > 1 ranks (or
--strong-minutes), `strong_scaling_e2e`: ONE 4 h recording sharded over the ranks, end to end.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

# MI355X dense MFMA peaks (MI355X_MICROARCH.md).  "f32s" contractions run fp32 arithmetic as 6 bf16 MFMA
# products per block (exact 3-way operand split, csrc/gemm_split.hip): their ALGORITHMIC peak is bf16 / 6.
# "mx" (r5, csrc/gemm_mx.hip): per 32 x 32 x 64 block 4 fp16 MFMAs of 8 passes + 2 block-scaled fp8 MFMAs of 16 passes = 64 passes
# where plain fp16 needs 32: algorithmic peak = fp16 dense peak / 2.
PEAK_TFLOPS = {"f32": 157.3, "bf16": 2500.0, "f32s": 2500.0 / 6.0, "f32h": 2500.0 / 3.0, "f16": 2500.0, "mx": 2500.0 / 2.0}


def prec_of(kernel_class: str, default: str = "f32") -> str:
    """arithmetic of a profiled kernel class, from its name; classes whose name carries no tag (conv01_fused: conv1 on the split
    MFMA forms of the engine mode) take `default`"""
    for tag in ("bf16", "f32s", "f32h", "mx", "f16"):
        if tag in kernel_class:
            return tag
    return "f32" if "gemm_f32_" in kernel_class else default
DTYPE_NOTE = {"f32": "f32 (fp32 MFMA v_mfma_f32_16x16x4_f32)",
              "f32s": "f32 (operands split exactly into 3 bf16 terms, 6 bf16 MFMA products, fp32 accumulate)",
              "f32h": "f32 (operands split into 2 fp16 terms with exact power-of-two scaling = 22 significant bits, 3 fp16 MFMA "
                      "products, fp32 accumulate: the error-corrected '3xFP16/3xTF32' scheme; kernels without an fp16 variant "
                      "use the 3-term bf16 split)",
              "bf16": "bf16 (bf16 MFMA operands, fp32 accumulate / residual stream / norms)",
              "f16": "f16 — REDUCED precision (BASELINE configs[4]): the f32h engine with every linear contraction of the segmentation "
                     "model as fp16 hi*hi + the two cross terms in fp8 e4m3 on the block-scaled matrix instruction "
                     "(v_mfma_scale_f32_32x32x64_f8f6f4, csrc/gemm_mx.hip: two thirds of f32h's matrix-pipe passes), the positional "
                     "conv and the ResNet stage 3-4 / stride-2 contractions at ONE fp16 term, fp32 accumulate, per-window "
                     "power-of-two scaling; attention, the conv stack and the fused BasicBlocks keep 2 fp16 terms; data, norms, "
                     "softmax, residual stream fp32"}
PEAK_HBM_GBS = 8000.0
TRAFFIC_SOURCE = ("committed rocprofv3 --pmc passes of this same command (separate FETCH_SIZE / WRITE_SIZE runs, gfx950 FETCH_SIZE x 2 "
                  "correction; scripts/final_measure_r5.sh -> profiles/) — not measured in this run")
# what holds the results of this path to the reference's (tests/ -m gpu, all through the C ABI; fixtures made by
# oracle/gen_golden.py from the reference's own code)
PARITY_NOTE = {
    "bar": "fp32 modes: max |dlogp| <= 1e-3 vs the reference-made goldens, identical u8 decisions, embeddings cos >= 0.9999, RTTM "
           "text identical; integer / index work bit-exact",
    "tests": ["test_seg_gpu.py (4 pruned configs x f32h/f32s/f32 vs reference goldens, plain + turn-taking; r4: dense wavlm_large "
              "and a checkpoint-embedded config vs reference-made goldens)", "test_emb_gpu.py (ResNet34 + fbank vs float64; r4: device "
              "fbank vs closed-form known answers; forwards capturable in a HIP graph)",
              "test_decisions_gpu.py (0 argmax flips on 102 144 frames: profiles/r4_decision_parity.json)",
              "test_f32h_grade_gpu.py (all 69 (N, K) of the r3 step vs float64: f32h <= 0.84 x the fp32-MFMA error, "
              "profiles/r3_f32h_grade_per_shape.json)",
              "test_ops_gpu.py (r4: fused BasicBlock kernels == two per-conv launches to 2e-6, == float64 to 1e-5)",
              "test_host_ref.py (host stage == the reference's own aggregate / speaker_count / to_diarization / reconstruct / "
              "Binarize)", "test_host.py (reference clustering incl. forced min/max speakers, max_num_embeddings)",
              "test_ops_gpu.py::test_linkage_centroid_30k_equals_scipy_golden", "test_pipeline_gpu.py (RTTM == golden, streaming)",
              "test_properties_gpu.py (batch / shard bit-invariance; r4: two handles on two streams == one)",
              "test_dist_gpu.py (2-rank pipeline RTTM == 1-GPU golden)"],
    "unpinned": ["kaldi fbank vs torchaudio (absent offline; r4: two independent float64 restatements + closed-form known answers agree "
                 "to 1e-11, == transformers.audio_utils to 1e-6)",
                 "pyannote.core 5.0.0 frame arithmetic / RTTM writer (absent offline)"]}
ALT_STEPS = 5          # timed steps of every comparison leg (other fp32 modes, reduced precision)
# the reduced mode against SURVEY 8d's reduced bar (max |dlogp| <= 5e-2, argmax >= 99.5 %, cos >= 0.999, DER delta <= 0.1 abs): the
# figures are MEASURED by the GPU tests (tests/test_seg_gpu.py::test_seg_f16_meets_the_reduced_bar_on_the_turn_taking_fixtures,
# tests/test_pipeline_gpu.py::test_der_between_arithmetic_modes) and committed under profiles/; bench.py quotes that file
REDUCED_PARITY_FILE = ROOT / "profiles" / "r5_reduced_mode_parity.json"


def other_roof(p, prec):
    """the OTHER roof of a matrix kernel class with declared algorithmic bytes: its rate against HBM, and which of the two roofs its
    algorithmic intensity puts lower (`binding_roof`).  The reduced contraction (half the matrix passes of plain fp16, same bytes as
    f32h) sits just on the HBM side of its ridge: 141 FLOP/B against 1250 / 8 = 156."""
    if p["bytes"] <= 0 or p["ms"] <= 0:
        return {}
    gbs = p["bytes"] / (p["ms"] * 1e-3) / 1e9
    intensity = p["flops"] / p["bytes"]
    ridge = PEAK_TFLOPS[prec] * 1e12 / (PEAK_HBM_GBS * 1e9)
    return {"alg_intensity_flop_per_byte": round(intensity, 1), "ridge_flop_per_byte": round(ridge, 1),
            "binding_roof": "mfma" if intensity >= ridge else "hbm",
            "alg_gbs": round(gbs, 1), "frac_of_hbm_peak": round(gbs / PEAK_HBM_GBS, 4)}


def reduced_parity():
    try:
        rec = json.loads(REDUCED_PARITY_FILE.read_text())
    except Exception:
        return {"meets_survey_8d_reduced_bar": None, "note": f"{REDUCED_PARITY_FILE.name} not found: run the GPU tests"}
    rec["source"] = f"profiles/{REDUCED_PARITY_FILE.name} (written by the GPU tests, committed)"
    return rec


from testkit.synth import synth_recording  # noqa: E402


# in-situ profiler class -> kernel symbol in the rocprofv3 tables (scripts/pmc_summary.py writes profiles/*.json)
# (a tuple = candidates in order: r6's kernels first, then the ones they replaced — older committed tables carry those)
PMC_SYMBOLS = {"conv0_ln_gelu": "conv0_kernel", "conv01_fused": ("conv01_ws_kernel", "conv01_fused_kernel"),
               "attention_relpos_f32s": "attn_split_kernel<true, 3>",
               "attention_relpos_f32h": ("attn_planes_kernel<true", "attn_split_kernel<true, 2>"),
               "attention_f32s": "attn_split_kernel<false, 3>",
               "attention_f32h": ("attn_planes_kernel<false", "attn_split_kernel<false, 2>"),
               "conv3x3_c32_f32s": "conv3x3_c32_split_kernel<3>", "conv3x3_c32_f32h": "conv3x3_c32_split_kernel<2>",
               "layernorm": "layernorm_v4_kernel<16", "row_stats": "row_stats_kernel<16>", "gate_ln_stats": "gate_stats_kernel",
               "ws_sum": "ws_sum_kernel", "stem_conv": "stem_conv_kernel", "glu_dwconv": "glu_dwconv_kernel",
               "stats_pool": "stats_pool_kernel", "pad_rows_split2": "pad_rows_split2_kernel",
               "resblock32_fused_f32h": "resblock32_fused_kernel<2>", "resblock64_ws_f32h": "resblock_ws_kernel<64, 2>",
               "resblock32_ws_f32h": "resblock_ws_kernel<32, 2>", "resblock32_fused_f16": "resblock32_fused_kernel<1>",
               "resblock64_ws_f16": "resblock_ws_kernel<64, 1>", "resblock32_ws_f16": "resblock_ws_kernel<32, 1>"}


class PowerSampler:
    """Board power and shader clock DURING the timed steps (rank 0, best effort): `rocm-smi --showpower --showclocks
    --showmaxpower --csv` polled from a thread.  The dominant contraction runs with the package at its power cap
    (profiles/r4_power_cap.txt) — this puts that evidence into the line the driver records.  Never raises;
    `result()` is None when rocm-smi is missing or answers nothing."""

    def __init__(self, period_s: float = 1.0, max_samples: int = 6, device=None):   # A/B on one box: 10 polls in a 4-step region cost 0.35 %
        import threading
        self.period, self.max = period_s, max_samples
        self.samples, self.cap = [], None
        # (r5) which rocm-smi card is the torch device: matched by PCI bus id; unmatched (or HIP_VISIBLE_DEVICES hiding
        # the mapping) = the first card, and the result says so
        self.card, self.card_matched = None, False
        try:
            import subprocess
            props = torch.cuda.get_device_properties(device if device is not None else torch.cuda.current_device())
            want = f"{getattr(props, 'pci_domain_id', 0):04x}:{props.pci_bus_id:02x}:{getattr(props, 'pci_device_id', 0):02x}".lower()
            out = subprocess.run(["/opt/rocm/bin/rocm-smi", "--showbus", "--csv"], capture_output=True, text=True, timeout=15).stdout
            for ln in out.splitlines():
                f = [c.strip() for c in ln.split(",")]
                if len(f) >= 2 and f[0].startswith("card") and f[1].lower().startswith(want):
                    self.card, self.card_matched = f[0], True
        except Exception:      # noqa: BLE001
            pass
        self._stop = threading.Event()
        self._th = threading.Thread(target=self._run, daemon=True)

    def _poll(self):
        import subprocess
        try:
            out = subprocess.run(["/opt/rocm/bin/rocm-smi", "--showpower", "--showclocks", "--showmaxpower", "--csv"],
                                 capture_output=True, text=True, timeout=15).stdout
            rows = [ln.split(",") for ln in out.splitlines() if ln.strip()]
            hdr = next(r for r in rows if r[0] == "device")
            row = next(r for r in rows if (r[0] == self.card if self.card else r[0].startswith("card")))
            self.card = self.card or row[0]
            col = {h.strip(): v for h, v in zip(hdr, row)}
            watts = float(next(v for h, v in col.items() if h.startswith("Current Socket Graphics Package Power")))
            sclk = next((v for h, v in col.items() if h.startswith("sclk clock speed")), "")
            mhz = int("".join(ch for ch in sclk if ch.isdigit()) or 0)
            cap = next((v for h, v in col.items() if h.startswith("Max Graphics Package Power")), None)
            if cap is not None:
                self.cap = float(cap)
            self.samples.append((watts, mhz))
        except Exception:      # noqa: BLE001 — evidence, not a dependency
            pass

    def _run(self):
        while not self._stop.is_set() and len(self.samples) < self.max:
            self._poll()
            self._stop.wait(self.period)

    def start(self):
        self._th.start()

    def stop(self):
        self._stop.set()
        self._th.join(timeout=20)

    def result(self):
        if not self.samples:
            return None
        w = [s[0] for s in self.samples]
        f = [s[1] for s in self.samples if s[1] > 0]
        return {"package_w": {"mean": round(sum(w) / len(w), 1), "max": round(max(w), 1)}, "cap_w": self.cap,
                "sclk_mhz": {"mean": round(sum(f) / len(f)) if f else None, "min": min(f) if f else None},
                "samples": len(w), "card": self.card, "card_matched_by_pci_bus_id": self.card_matched,
                "source": "rocm-smi polled from a thread while the timed steps ran (whole pipeline: every kernel, not only the "
                          "contraction; back to back the contraction alone holds 1400 W of 1400 W at 1.84-1.92 GHz, "
                          "profiles/r4_power_cap.txt)"}


def pmc_table(args, precision=None):
    """HBM bytes per launch / MfmaUtil per kernel from the committed rocprofv3 --pmc passes of this same command
    (separate passes per counter, gfx950 FETCH_SIZE correction: scripts/pmc_traffic.py, scripts/pmc_mfma.py).
    bench.py cannot run rocprofv3 on itself, so the table is read from profiles/ and only when the workload matches
    the one the passes were taken on; otherwise `traffic` is null."""
    found = sorted((ROOT / "profiles").glob(f"r*_pmc_{precision or args.precision}_30min_b{args.batch}.json"))   # newest round last
    if not found or args.minutes != 30.0 or args.model != "wavlm_large_s80_md" or args.window != 8.0:
        return None
    table = json.loads(found[-1].read_text())
    table["_file"] = f"profiles/{found[-1].name}"
    return table


def rocprof_trace_name(args):
    """the committed `rocprofv3 --kernel-trace --stats` summary of this same command whose average duration of the dominant
    kernel `roofline.avg_launch_ms` is to be compared with (newest round last)"""
    found = sorted((ROOT / "profiles").glob(f"r*_kernel_stats_{args.precision}_30min_b{args.batch}.csv"))
    if not found or args.minutes != 30.0 or args.model != "wavlm_large_s80_md" or args.window != 8.0:
        return None
    return f"profiles/{found[-1].name}"


def pmc_lookup(table, kernel_class: str, field: str):
    if not table:
        return None
    key = None
    if kernel_class.startswith("gemm_mx_"):          # gemm_mx_kernel<BM, BN, WGM, WGN, S, OCC, RPF>
        bm, bn = kernel_class[len("gemm_mx_"):].split("_")[0].split("x")
        for k in table:
            if k.startswith("gemm_mx_kernel<"):
                targs = [t.strip() for t in k[len("gemm_mx_kernel<"):].rstrip(">").split(",")]
                if len(targs) >= 2 and targs[0] == bm and targs[1] == bn:
                    return table[k].get(field)
        return None
    for tag, planes in (("gemm_f32h_pre_", 2), ("gemm_f32s_pre_", 3), ("gemm_f32h_", 2), ("gemm_f32s_", 3), ("gemm_f16_pre_", 1), ("gemm_f16_", 1)):
        if kernel_class.startswith(tag):
            bm, bn = kernel_class[len(tag):].split("x")
            sym = "gemm_split_pre_kernel" if "_pre_" in tag else "gemm_split_kernel"
            for k in table:     # template arguments: <BM, BN, WGM, WGN, S, NP[, OCC]>
                if k.startswith(sym + "<"):
                    targs = [t.strip() for t in k[len(sym) + 1:].rstrip(">").split(",")]
                    if len(targs) >= 6 and targs[0] == bm and targs[1] == bn and targs[5] == str(planes):
                        key = k
                        break
            break
    else:
        syms = PMC_SYMBOLS.get(kernel_class)
        syms = (syms,) if isinstance(syms, str) else (syms or ())
        key = next((k for sym in syms for k in table if k.startswith(sym)), None)
    return table[key].get(field) if key else None


def cpu_baseline(seg_cfg, sd, esd, window: int, step_s: float, budget_windows: int = 32, clustering_args=None):
    """CPU timing of the WHOLE pipeline's arithmetic on a bounded sample (outside every timed region): the `budget_windows`
    consecutive windows of a short synthetic recording through segmentation (one batch of 32, the reference's inference batch),
    hard decisions, median filter, overlap-excluded masks, the embedding stage AS THE REFERENCE EXECUTES IT — one ResNet34 pass per
    (window, local speaker), batches of 32 pairs (PA/pipelines/speaker_diarization.py:295-353) — and the host stage: speaker
    counting, agglomerative clustering, constrained assignment, reconstruction, Binarize, RTTM.
    kind = "reference" when /root/reference is present (build container): the reference's OWN modules — wav2vec2_model +
    ConformerEncoder wired as model_wavlm_conformer.py:58-76,250-262, wespeaker/resnet.py ResNet34 (strict state_dict loads,
    oracle/gen_golden.py), its own AgglomerativeClustering — with the oracle's fbank in front of the ResNet (torchaudio is
    absent) and the oracle's aggregation loops behind the clustering.  On the GPU box there is no /root/reference: kind = "port",
    the oracle restatements of the same modules (oracle/seg_model.py, emb_model.py, clustering_port.py, host_stage.py)."""
    import math
    import types
    import numpy as np
    from scipy.ndimage import median_filter
    from oracle import clustering_port, emb_model, gen_golden, host_stage, seg_model
    from oracle.pipeline import slide_windows
    clu = clustering_args or {"ahc_threshold": 0.1, "min_cluster_size": 13, "min_speakers": 1, "max_speakers": 20}
    threads = torch.get_num_threads()
    step = int(round(step_s * 16000))
    n_samples = window + (budget_windows - 1) * step
    wave = synth_recording(n_samples, seed=99)
    kind = "port"
    ref_cl = None
    if gen_golden.REF.exists():
        try:
            import warnings
            fwd = gen_golden.build_reference_seg(seg_cfg, sd)
            resnet, _ = gen_golden.load_reference_resnet()
            net = resnet.ResNet34(80, 256, pooling_func="TSTP", two_emb_layer=False)
            net.load_state_dict({k[len("resnet."):]: v for k, v in esd.items()}, strict=True)
            net.eval()
            ref_cl = gen_golden.load_reference_clustering()
            kind = "reference"
        except Exception as e:           # an incomplete reference tree: fall back to the port, say so
            print(f"[bench] reference modules not importable ({type(e).__name__}: {e}); cpu_baseline uses the oracle", file=sys.stderr)
    t0 = time.perf_counter()
    chunks = slide_windows(wave, window, step)                      # PA/core/inference.py:282-299
    C = chunks.shape[0]
    with torch.inference_mode():
        if kind == "reference":
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                logp, _ = fwd(chunks)
        else:
            logp = seg_model.seg_forward(sd, seg_cfg, chunks)
        seg = seg_model.to_multilabel(logp, seg_cfg).numpy().astype(np.float32)
        seg = median_filter(seg, size=(1, 11, 1), mode="reflect")   # diarizen/pipelines/inference.py:131-132
        L, S = seg.shape[1], seg.shape[2]
        min_num_frames = math.ceil(L * 400 / window)                # speaker_diarization.py:274-278
        clean = seg * (np.sum(seg, axis=2, keepdims=True) < 2)
        masks = np.where((clean.sum(1, keepdims=True) > min_num_frames), clean, seg)       # [C, L, S]
        pairs = [(c, s_) for c in range(C) for s_ in range(S)]
        emb = np.zeros((C, S, 256), dtype=np.float32)
        for b0 in range(0, len(pairs), 32):                        # embedding batch size 32 (speaker_diarization.py:320-353)
            pb = pairs[b0:b0 + 32]
            wv = torch.stack([chunks[c] for c, _ in pb])
            mk = torch.from_numpy(np.stack([masks[c, :, s_] for c, s_ in pb]))
            if kind == "reference":
                e = net(emb_model.compute_fbank(wv), weights=mk)
                e = e[-1] if isinstance(e, (tuple, list)) else e
            else:
                e = emb_model.emb_forward(esd, wv, mk)
            for (c, s_), v in zip(pb, e.numpy()):
                emb[c, s_] = v
    t_dev = time.perf_counter()
    segu = seg.astype(np.uint8)
    if kind == "reference":
        ahc = ref_cl.AgglomerativeClustering(metric="cosine")
        ahc.method, ahc.threshold, ahc.min_cluster_size = "centroid", clu["ahc_threshold"], clu["min_cluster_size"]
        hard, _, _ = ahc(embeddings=emb.copy(), segmentations=types.SimpleNamespace(data=seg), min_clusters=clu["min_speakers"],
                         max_clusters=clu["max_speakers"])
    else:
        hard = clustering_port.agglomerative(emb, seg, clu["ahc_threshold"], clu["min_cluster_size"], clu["min_speakers"],
                                             clu["max_speakers"])
    rttm = host_stage.host_stage(segu, hard, window / 16000.0, step_s * 16000.0 / window, clu["max_speakers"], "cpu_baseline")
    dt = time.perf_counter() - t0
    audio_s = n_samples / 16000.0
    what = ("the reference's own wav2vec2_model + ConformerEncoder + ResNet34 modules and AgglomerativeClustering (imported from "
            "/root/reference)" if kind == "reference" else
            "oracle restatements of the reference modules and of its clustering (no /root/reference on this box)")
    return {"value": round(audio_s / dt, 4), "unit": "audio-seconds/s", "cores": threads,
            "kind": kind,
            "sample": f"{C} consecutive windows of {window} samples = a {audio_s:.1f} s recording through the WHOLE pipeline: {what}: "
                      f"seg forward (batch {C}) + median filter + masks + one ResNet34 pass per (window, speaker) in batches of 32 "
                      f"pairs + speaker counting + AHC + assignment + reconstruction + RTTM ({len(rttm.splitlines())} lines), fp32 "
                      f"torch CPU, {dt:.1f} s of which host stage {dt - (t_dev - t0):.2f} s",
            "device_part_s": round(t_dev - t0, 2), "host_part_s": round(dt - (t_dev - t0), 3)}


def shard_slice(num_samples: int, window: int, step: int, rank: int, world: int):
    """strong scaling: rank -> (first window, one-past-last window, first sample, samples incl. the window-length halo)"""
    from diarizen_amd.dist import shard_range
    from diarizen_amd.inference import window_plan
    n, last = window_plan(num_samples, window, step)
    c0, c1 = shard_range(n + int(last), rank, world)
    if c1 <= c0:
        return c0, c1, 0, 0
    return c0, c1, c0 * step, (c1 - c0 - 1) * step + window


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, seg, emb, tracks) -> dict:
    """--dump-outputs: what the last timed step handed its caller, as DIR/<name>.npy — `segmentations` (the u8 hard decisions
    [windows, frames, speakers] as float32), `embeddings` (float32 [windows, speakers, dim]; full stage only) and `diarization`
    (float64 [segments, 3]: start s, end s, speaker index into the sorted labels, in RTTM order; full stage only).  Past 64 MB
    in all, a seeded sample of the windows (the same rows of both arrays) is written, with their indices in `window_index`."""
    import numpy as np
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    arrays = {"segmentations": seg.numpy().astype(np.float32)}
    if emb is not None:
        arrays["embeddings"] = emb.numpy().astype(np.float32)
    if tracks is not None:
        arrays["diarization"] = np.asarray(tracks, dtype=np.float64).reshape(-1, 3)
    per_window = sum(a[0].nbytes for k, a in arrays.items() if k != "diarization" and len(a))
    fixed = arrays["diarization"].nbytes if "diarization" in arrays else 0
    n = len(arrays["segmentations"])
    if per_window * n + fixed > DUMP_LIMIT_BYTES:
        keep = max(1, (DUMP_LIMIT_BYTES - fixed - 8 * n) // per_window)
        idx = np.sort(np.random.default_rng(0).choice(n, size=min(n, keep), replace=False))
        for k in ("segmentations", "embeddings"):
            if k in arrays:
                arrays[k] = arrays[k][idx]
        arrays["window_index"] = idx.astype(np.float64)
    for k, a in arrays.items():
        np.save(out_dir / f"{k}.npy", np.ascontiguousarray(a))
    return {k: list(a.shape) for k, a in arrays.items()}


def batches_note(n_windows: int, batch: int) -> str:
    nb = max(1, -(-n_windows // batch))
    return f"{nb} balanced launches of <= {-(-n_windows // nb)} windows (max batch {batch})"


def run_mode(cfg, sd, esd, wave, args, window, precision, full, dev, profile=False):
    """one untimed + ALT_STEPS timed steps of the DEVICE hot path of the same workload in another arithmetic mode (reported
    beside the headline; compare with `device_value`).  profile=True: the in-situ HIP-event profiler runs inside those steps
    and the per-class records come back too (the reduced mode's own roofline entry)."""
    from diarizen_amd import _lib
    from diarizen_amd.configs import RESNET34
    from diarizen_amd.engine import Engine
    from diarizen_amd.inference import WindowRunner
    eng = Engine(cfg, sd, RESNET34, esd, max_batch=args.batch, max_samples=window, precision=precision, device=dev)
    r = WindowRunner(eng, args.window, 0.1, args.batch)

    def one():
        res = r.run(wave, with_embeddings=full)
        _ = (res.segmentations.cpu(), res.embeddings.cpu()) if full else res.segmentations.cpu()
    one()                                   # warm-up (allocations, tables)
    if profile:
        _lib.profile_enable(True)
        one()
        launches = sum(p["launches"] for p in _lib.profile_collect())
        _lib.profile_reserve(2 * launches * ALT_STEPS + 1024)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for _ in range(ALT_STEPS):
        one()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t1) / ALT_STEPS
    prof = _lib.profile_collect() if profile else None
    if profile:
        _lib.profile_enable(False)
    eng.close()
    return (dt, prof) if profile else dt


def pipeline_conf(args, cfg):
    return {"model": {"path": "diarizen.models.eend.model_wavlm_conformer.Model",
                      "args": {"wavlm_src": args.model, "wavlm_layer_num": cfg.wavlm_layer_num,
                               "wavlm_feat_dim": cfg.embed_dim, "chunk_size": int(args.window)}},
            "inference": {"args": {"seg_duration": args.window, "segmentation_step": 0.1, "batch_size": args.batch,
                                   "apply_median_filtering": True}},
            "clustering": {"args": {"method": "AgglomerativeClustering", "min_speakers": 1, "max_speakers": 20,
                                    "ahc_criterion": "distance", "ahc_threshold": 0.1, "min_cluster_size": 13}}}


def e2e_leg(args, dev, wave_host, sd, esd):
    """BASELINE configs[2] as it is worded — segmentation + embedding + AHC: `--e2e-steps` timed passes of the whole
    DiariZenPipeline (host -> HBM upload, device stage, D2H, then speaker counting / AHC / assignment / reconstruction /
    RTTM on the host) over the same recording and the same weights as the headline steps; mean over the passes."""
    import copy
    import numpy as np
    from diarizen_amd.configs import get_seg_config
    from diarizen_amd.pipeline import DiariZenPipeline
    cfg = get_seg_config(args.model)
    pipe = DiariZenPipeline(None, None, config=copy.deepcopy(pipeline_conf(args, cfg)), device=dev, precision=args.precision,
                            seg_state=sd, emb_state=esd)
    x = np.ascontiguousarray(wave_host.numpy())
    seg, emb = pipe.device_stage(x)          # untimed: allocations / tables
    ann = pipe.host_stage(seg, emb, "bench")
    K = max(1, args.e2e_steps)
    dev_s = host_s = 0.0
    per = []
    for _ in range(K):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        seg, emb = pipe.device_stage(x)
        t1 = time.perf_counter()
        ann = pipe.host_stage(seg, emb, "bench")
        t2 = time.perf_counter()
        dev_s += t1 - t0
        host_s += t2 - t1
        per.append(round(t2 - t0, 4))
    dev_s /= K
    host_s /= K
    audio_s = len(x) / 16000.0
    active = int((seg.sum(1) > 0).sum())
    # the same object over a CORPUS (DiariZenPipeline.diarize_many, the reference's `for audio_file in audio_f:` loop,
    # diarizen/pipelines/inference.py:365-368): K + 1 in-memory 16-bit WAV files of the recording, decode + upload + device
    # stage of file i+1 beside the host stage of file i
    import io
    import wave as _wave
    buf = io.BytesIO()
    with _wave.open(buf, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes((np.clip(x, -1.0, 1.0) * 32767.0).astype("<i2").tobytes())
    blob = buf.getvalue()
    corpus = {}
    for overlap in (False, True):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n_done = sum(1 for _ in pipe.diarize_many([blob] * (K + 1), sess_names=[f"bench{i}" for i in range(K + 1)], overlap=overlap))
        torch.cuda.synchronize()
        corpus["overlapped" if overlap else "serial"] = round(audio_s * n_done / (time.perf_counter() - t0), 1)
    pipe.close()      # (r5) both engine handles now: the pipeline object sits in a reference cycle (runner -> engine factory -> pipeline)
                      # and would keep its ~180 GB until the cycle collector runs
    return {"audio_seconds_per_s": round(audio_s / (dev_s + host_s), 1), "steps": K, "s_per_step": per,
            "device_s": round(dev_s, 4), "host_s": round(host_s, 4), "upload_included": True,
            "speakers": len(ann.labels()), "rttm_lines": len(ann.to_rttm().splitlines()),
            "active_window_speakers": active,
            "corpus_audio_seconds_per_s": corpus,
            "corpus_note": f"DiariZenPipeline.diarize_many over {K + 1} in-memory 16-bit WAV copies of the recording (WAV decode + upload + "
                           "device stage + host stage each): serial = one after the other as the reference's loop, overlapped = the host "
                           "stage of file i in a worker thread beside the decode + device stage of file i+1",
            "note": "mean of `steps` passes of DiariZenPipeline: host->HBM upload + segmentation + masks + embeddings + D2H "
                    "(device_s), then host counting + AHC (centroid linkage) + constrained assignment + reconstruction + "
                    "RTTM (host_s); same recording and seeded turn-taking weights as the headline steps"}


def config1_leg(args, dev):
    """BASELINE configs[1]: wavlm-base-s80, segmentation only, 5 s windows, ONE batch of 32 at a time (the reference's own
    configuration for that line), driver-timed beside the headline.  A pass = the 3591 windows of a 30-min recording
    in 113 launches of <= 32; `streams` > 1 (default 3: 3205 / 4192 / 4623 / 4167 audio-s/s at 1 / 2 / 3 / 4, gpurun r4f) runs consecutive batches on separate engine handles / HIP streams,
    because a 32-window launch (7968 rows) under-fills 256 CUs and its 113 kernels are launch-granularity bound."""
    from diarizen_amd.configs import RESNET34, get_seg_config
    from diarizen_amd.engine import Engine
    from diarizen_amd.inference import WindowRunner
    from testkit.weights import turn_taking_state_dict
    name, win_s, batch = "wavlm_base_s80_md", 5.0, 32
    cfg = get_seg_config(name)
    sd = turn_taking_state_dict(cfg, 0)
    window = int(win_s * 16000)
    nstream = max(1, args.config1_streams)
    wave = synth_recording(int(args.config1_minutes * 60 * 16000), seed=1).to(dev)
    out = {}
    for ns in sorted({1, nstream}):
        engines = [Engine(cfg, sd, None, None, max_batch=batch, max_samples=window, precision=args.precision, device=dev)
                   for _ in range(ns)]
        runners = [WindowRunner(e, win_s, 0.1, batch) for e in engines]
        streams = [torch.cuda.Stream(device=dev) for _ in range(ns)] if ns > 1 else [torch.cuda.current_stream(dev)]
        views = runners[0].windows_view(wave)
        C = views.shape[0]

        def one():
            torch.cuda.synchronize()
            segs = []
            for i, s0 in enumerate(range(0, C, batch)):
                k = i % ns
                with torch.cuda.stream(streams[k]):
                    r = runners[k].run_views(views, s0, min(s0 + batch, C), with_embeddings=False)
                    segs.append(r.segmentations)
            torch.cuda.synchronize()
            return torch.cat(segs).cpu()
        one()
        t0 = time.perf_counter()
        for _ in range(args.config1_steps):
            res = one()
        dt = (time.perf_counter() - t0) / args.config1_steps
        for e in engines:
            e.close()
        out[ns] = {"audio_seconds_per_s": round(wave.numel() / 16000.0 / dt, 1), "windows_per_s": round(C / dt, 1),
                   "ms_per_batch_of_32": round(dt * 1e3 / -(-C // batch), 4), "streams": ns, "steps": args.config1_steps}
    best = max(out.values(), key=lambda v: v["audio_seconds_per_s"])
    return {"workload": f"{name} segmentation only, {win_s:g} s windows, batch {batch}, {C} windows of a {args.config1_minutes:g} min "
                        f"synthetic recording per step (BASELINE configs[1]); unprofiled",
            **best, "by_streams": {str(k): v["audio_seconds_per_s"] for k, v in out.items()},
            "alg_gflop_per_window": 15.21,
            "alg_tflops": round(best["windows_per_s"] * 15.21e-3, 1)}


def strong_leg(args, dev, rank, world, minutes):
    """BASELINE configs[3]: ONE recording of `minutes` whose windows are sharded over the ranks, END TO END — each rank
    reads + uploads only its slice, runs segmentation + embeddings on its windows, one RCCL all-gather per tensor, then
    rank 0 runs the host stage (counting, AHC, assignment, reconstruction, RTTM).  The serial part (gather + host) is
    reported next to the sharded part so that Amdahl's bound on the end-to-end speed-up is visible in the line."""
    import copy
    import torch.distributed as dist
    from diarizen_amd.configs import get_seg_config
    from diarizen_amd.pipeline import DiariZenPipeline
    from testkit.weights import emb_state_dict, turn_taking_state_dict
    cfg = get_seg_config(args.model)
    pipe = DiariZenPipeline(None, None, config=copy.deepcopy(pipeline_conf(args, cfg)), device=dev, precision=args.precision,
                            seg_state=turn_taking_state_dict(cfg, 0), emb_state=emb_state_dict(0))
    # the recording is a real RIFF file on local disk, so the timed region pays the byte-range decode a deployment pays
    # (audio.WavSource), not the synthesis: every rank synthesises the samples of ITS window block (1 / world of the
    # work) and writes them at their byte offset of one shared 16-bit PCM file; blocks overlap by one window of halo
    # with identical data
    import struct
    from diarizen_amd import dist as dz_dist
    from diarizen_amd.audio import WavSource
    from testkit.synth import synth_recording_range
    total = int(minutes * 60 * 16000)
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"),      # one name for all ranks of THIS job
                        f"dzn_strong_{int(minutes)}min_{os.getuid()}_{os.environ.get('MASTER_PORT', '0')}.wav")
    if rank == 0:
        with open(path, "wb") as f:
            f.write(b"RIFF" + struct.pack("<I", 36 + 2 * total) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, 16000, 32000, 2, 16)
                    + b"data" + struct.pack("<I", 2 * total))
            f.truncate(44 + 2 * total)
    if world > 1:
        dist.barrier()
    r = pipe._runner
    c0, c1 = dz_dist.shard_range(r.num_windows(total), rank, world)
    lo, n = c0 * r.step, ((c1 - c0 - 1) * r.step + r.window if c1 > c0 else 0)
    n = max(0, min(n, total - lo))
    if n:
        x = synth_recording_range(lo, n, total=total)
        with open(path, "r+b") as f:
            f.seek(44 + 2 * lo)
            f.write((x.numpy() * 32767.0).astype("<i2").tobytes())
        del x
    if world > 1:
        dist.barrier()
    src = WavSource(path)
    best = None
    for _ in range(2):                       # first pass warms allocations / tables / RCCL channels
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        seg, emb = pipe.device_stage(src)    # slice read + upload + device stage + all-gather (+ D2H)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        t1 = time.perf_counter()
        ann = pipe.host_stage(seg, emb, "bench") if rank == 0 else None
        t2 = time.perf_counter()
        best = (t1 - t0, t2 - t1, ann)
    dev_s, host_s, ann = best
    if world > 1:
        tt = torch.tensor([dev_s], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dev_s = tt.item()
    if rank != 0:
        return None
    audio_s = src.num_samples / 16000.0
    try:
        os.remove(path)
    except OSError:
        pass
    return {"workload": f"{args.model} full pipeline, ONE {minutes:g} min synthetic recording, {seg.shape[0]} windows sharded over "
                        f"{world} rank(s) (contiguous blocks), all-gather, host stage on rank 0",
            "scaling": "strong", "n_gpus": world, "audio_s": audio_s,
            "sharded_s": round(dev_s, 3), "serial_host_s": round(host_s, 3),
            "e2e_audio_seconds_per_s": round(audio_s / (dev_s + host_s), 1),
            "device_only_audio_seconds_per_s": round(audio_s / dev_s, 1),
            "amdahl_serial_frac": round(host_s / (dev_s + host_s), 4),
            # (r6) what the measured components allow at more GPUs: the sharded part (range decode + upload +
            # device stage of a contiguous window block) divides by N, the host stage of the ONE recording stays on rank 0
            "projected_from_this_run": (None if world != 1 else {
                f"{n}_gpus": {"e2e_s": round(dev_s / n + host_s, 3), "audio_seconds_per_s": round(audio_s / (dev_s / n + host_s), 1),
                              "efficiency": round((dev_s + host_s) / (n * (dev_s / n + host_s)), 3)} for n in (2, 4, 8)}),
            "projection_note": "PROJECTED, not measured: T(N) = sharded_s / N + serial_host_s from this run's two figures (blocks are "
                               "balanced to one window; the all-gather moves 5.7 KB per window: 13 MB at 4 h)" if world == 1 else None,
            "speakers": len(ann.labels()), "rttm_lines": len(ann.to_rttm().splitlines()),
            "note": "sharded_s = max over ranks of [byte-range decode of the rank's block of a 16-bit PCM file + upload + segmentation + embeddings + RCCL all-gather + D2H]; "
                    "serial_host_s = rank 0's counting + AHC + assignment + reconstruction + RTTM; seeded turn-taking weights"}


def launcher_command(args, argv, port: int):
    """the command `--gpus N` re-executes itself through: one rank per GPU of this node, rendezvous on 127.0.0.1"""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
            "--master-addr", "127.0.0.1", "--master-port", str(port), str(Path(__file__).resolve()), *argv]


def self_launch(args, argv, one_device: bool) -> int:
    """`python bench.py --gpus N` with no launcher around it: check that N devices exist, then start the N ranks.
    Returns the launcher's exit code (rank 0 prints the JSON line on the inherited stdout)."""
    import socket
    import subprocess
    if not args.rendezvous_check:
        if not torch.cuda.is_available():
            print("bench.py needs a HIP device (the product has no CPU path)", file=sys.stderr)
            return 2
        ndev = torch.cuda.device_count()
        if ndev < args.gpus and not one_device:
            print(f"bench.py: --gpus {args.gpus} needs {args.gpus} visible HIP devices, torch.cuda.device_count() = {ndev}; "
                  f"refusing to time fewer ranks than asked for (DZN_BENCH_ONE_DEVICE=1 rehearses the N-rank path on one "
                  f"device through gloo)", file=sys.stderr)
            return 2
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL across processes needs it on this driver
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // max(args.gpus, 1))))
    return subprocess.call(launcher_command(args, argv, port), env=env)


def visible_device_ids():
    """the physical device list this process tree may see, as HIP numbers it: HIP_VISIBLE_DEVICES (or ROCR_ / CUDA_) entries in
    order - torch's `cuda:i` is entry i.  None = no restriction (cuda:i is physical device i)."""
    for var in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None and v.strip() != "":
            return [t.strip() for t in v.split(",") if t.strip() != ""], var
    return None, None


def rendezvous_check(args, rank: int, world: int):
    """`--rendezvous-check`: the N-rank job WITHOUT a GPU.  The ranks `--gpus N` started form
    ONE gloo group of N and every rank contributes to an all-reduce; then the dry run of what the timed job does per rank:
    rank -> `cuda:LOCAL_RANK` -> physical device under the HIP_VISIBLE_DEVICES permutation in force (must be N distinct
    devices), the strong leg's window blocks and sample ranges of the 4 h recording (must tile it, halo included), and the
    path's one exchange - the packed all-gather of diarizen_amd/dist.py with the partition check - on a stand-in payload whose
    values are the global window indices.  Rank 0 prints what came up; a violated check is a non-zero exit on every rank."""
    import torch.distributed as dist
    from diarizen_amd.dist import gather_windows, shard_range
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29517")          # only reached without a launcher at --gpus 1
    os.environ.setdefault("RANK", str(rank))
    os.environ.setdefault("WORLD_SIZE", str(world))
    dist.init_process_group(backend="gloo")
    if dist.get_world_size() != args.gpus:
        raise SystemExit(f"process group has {dist.get_world_size()} ranks, --gpus {args.gpus}")
    t = torch.tensor([float(rank + 1)])
    dist.all_reduce(t)
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    ids, var = visible_device_ids()
    if ids is not None and local_rank >= len(ids):
        raise SystemExit(f"bench.py: LOCAL_RANK {local_rank} has no entry in {var}={','.join(ids)}")
    sr, window, step = 16000, int(args.window * 16000), int(round(0.1 * args.window * 16000))
    total = int((args.strong_minutes if args.strong_minutes else 240.0) * 60 * sr)
    c0, c1, s0, ns = shard_slice(total, window, step, rank, world)
    mine = {"rank": rank, "local_rank": local_rank, "pid": os.getpid(), "torch_device": f"cuda:{local_rank}",
            "physical_device": ids[local_rank] if ids is not None else str(local_rank),
            "windows": [c0, c1], "samples": [s0, s0 + ns]}
    ranks = [None] * world
    dist.all_gather_object(ranks, mine)
    C = ranks[-1]["windows"][1]
    # the exchange on a stand-in payload: u8 decisions [c, 3, 4] and f32 embeddings [c, 4, 2] that carry the window index
    idx = torch.arange(c0, c1)
    seg = (idx % 251).to(torch.uint8).view(-1, 1, 1).expand(c1 - c0, 3, 4).contiguous()
    emb = idx.to(torch.float32).view(-1, 1, 1).expand(c1 - c0, 4, 2).contiguous()
    gs, ge = gather_windows(seg, emb, expected_total=C, to_host=True)
    problems = []
    phys = [r["physical_device"] for r in ranks]
    if len(set(phys)) != world:
        problems.append(f"ranks share a physical device: {phys}")
    if [r["windows"] for r in ranks] != [list(shard_range(C, r, world)) for r in range(world)] or ranks[0]["windows"][0] != 0:
        problems.append("window blocks are not the block partition of the recording")
    for r in ranks:
        w0, w1 = r["windows"]
        if w1 > w0 and (r["samples"][0] != w0 * step or r["samples"][1] < min((w1 - 1) * step + window, total)):
            problems.append(f"rank {r['rank']}: sample range {r['samples']} does not cover its windows {r['windows']}")
    if not (torch.equal(ge[:, 0, 0], torch.arange(C, dtype=torch.float32)) and gs.shape == (C, 3, 4)):
        problems.append("gathered payload is not in window order")
    if rank == 0:
        print(json.dumps({"rendezvous": "ok" if not problems else "FAILED", "n_gpus": world, "backend": "gloo",
                          "sum_of_rank_ids": t.item(), "visible_devices_var": var, "ranks": ranks,
                          "strong_leg_windows": C, "gathered_windows": int(gs.shape[0]), "problems": problems}))
    dist.barrier()
    dist.destroy_process_group()
    if problems:
        raise SystemExit("bench.py --rendezvous-check: " + "; ".join(problems))


def strong_minutes(args, world: int) -> float:
    """length of the ONE recording of the strong-scaling leg: --strong-minutes, else 240 at N > 1 ranks and none at one"""
    return args.strong_minutes if args.strong_minutes is not None else (240.0 if world > 1 else 0.0)


def extra_legs(args, world: int) -> set:
    """the legs a run measures besides its timed steps.  A plain run has none: it sets up, warms up, times the steps, dumps and
    prints the line (`roofline` / `kernels` / `power` are recorded while the timed steps run, so they stay with them).  --full
    adds the legs that take runs of their own, as they ran before the option existed, each trimmed by its --no-* flag."""
    if not args.full:
        return set()
    seg_emb = args.stage == "full"
    legs = {"serial"}
    if world == 1 and not args.no_alt:
        if args.precision in ("f32h", "f32s"):
            legs.add("other_modes")
        if args.streams == 1:
            legs.add("two_streams")
    if world == 1 and seg_emb and not args.no_e2e and args.minutes <= 60:
        legs.add("e2e")
    if strong_minutes(args, world) > 0 and seg_emb and not args.no_e2e:
        legs.add("strong")
    if world == 1 and not args.no_config1:
        legs.add("config1")
    if world == 1 and seg_emb and not args.no_cpu_baseline:
        legs.add("cpu_baseline")
    return legs


def arg_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--precision", default=os.environ.get("DZN_BENCH_PRECISION", "f32h"),
                    choices=["f32h", "f32s", "f32", "bf16", "f16"],
                    help="f32h (default), f32s and f32 are fp32 arithmetic held to the same strict parity tolerance: "
                         "f32h = 2-term fp16 split / 3 MFMA products, f32s = 3-term bf16 split / 6 products, "
                         "f32 = the fp32 MFMA instruction")
    ap.add_argument("--minutes", type=float, default=30.0)
    ap.add_argument("--window", type=float, default=8.0)
    ap.add_argument("--batch", type=int, default=576,
                    help="maximum windows per launch (the runner balances: 2241 windows -> 4 launches of 561; r4 sweep on one box: "
                         "384 / 576 / 768 / 1152 -> 1062 / 1043 / 1042 / 1036 ms per step; 576 keeps two handles of 68 GB each (91 GB with the per-layer buffers of the deferred layer-weighted sum) "
                         "and an even number of launches for the two-stream pipeline)")
    ap.add_argument("--streams", type=int, default=1,
                    help="engine handles / HIP streams that consecutive batches of a step alternate over (WindowRunner "
                         "extra_engines); the in-situ per-kernel profiler needs 1 (kernel durations are not separable when "
                         "two streams share the device)")
    ap.add_argument("--model", default="wavlm_large_s80_md")
    ap.add_argument("--stage", default="full", choices=["full", "seg"],
                    help="seg = segmentation-only (BASELINE configs[1]: --model wavlm_base_s80_md --window 5 "
                         "--batch 32 --stage seg)")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="weak: every rank owns its own recording of --minutes; strong (BASELINE configs[3]): ONE "
                         "recording of --minutes whose windows are sharded over the ranks (each rank uploads only its "
                         "slice + one window of halo)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--no-power", action="store_true", help="do not poll rocm-smi (package power, sclk) during the timed steps")
    ap.add_argument("--no-alt", action="store_true", help="skip the extra steps in the other fp32 modes")
    ap.add_argument("--no-overlap", action="store_true",
                    help="run every step's host stage serially behind its device stage (the steps of the first r5 runs)")
    ap.add_argument("--no-e2e", action="store_true", help="skip the end-to-end (device + host AHC) leg")
    ap.add_argument("--e2e-steps", type=int, default=3, help="timed passes of the end-to-end leg (upload + device + host AHC)")
    ap.add_argument("--no-config1", action="store_true", help="skip the BASELINE configs[1] leg (base-s80, 5 s x 32, segmentation only)")
    ap.add_argument("--only-config1", action="store_true", help="run just the BASELINE configs[1] leg and print its object")
    ap.add_argument("--config1-steps", type=int, default=2)
    ap.add_argument("--config1-minutes", type=float, default=30.0)
    ap.add_argument("--config1-streams", type=int, default=3,
                    help="engine handles / HIP streams that consecutive 32-window batches of the configs[1] leg alternate over")
    ap.add_argument("--weights", default="turn_taking", choices=["turn_taking", "plain"],
                    help="turn_taking (default): seeded weights whose decisions look like turn taking (both mask branches of "
                         "get_embeddings, silent windows, many powerset classes); plain: seeded N(0,1) init (one class per frame)")
    ap.add_argument("--rendezvous-check", action="store_true",
                    help="launcher self-test (runs without a GPU): bring up the --gpus N ranks on gloo, all-reduce, print "
                         "{n_gpus, ranks} and exit")
    ap.add_argument("--strong-minutes", type=float, default=None,
                    help="length of the ONE recording of the strong-scaling end-to-end leg (BASELINE configs[3]: 240); "
                         "default: 240 when --gpus > 1, off at 1 GPU; runs with --full")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (decisions, embeddings, diarization) as "
                         "DIR/<name>.npy on rank 0, for output-for-output comparison of two builds (bench.py:dump_outputs)")
    ap.add_argument("--full", action="store_true",
                    help="also run every leg that takes runs of its own (extra_legs): the serial steps, the other arithmetic "
                         "modes, two streams, e2e, the strong-scaling leg, config1 and cpu_baseline; without it a run only sets "
                         "up, warms up, times the steps, dumps and prints the line")
    return ap


def main():
    args = arg_parser().parse_args()

    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("--steps must be >= 1 and --warmup >= 0")
    one_device = bool(os.environ.get("DZN_BENCH_ONE_DEVICE"))    # rehearsal only: N ranks on device 0 (gloo staging)
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        raise SystemExit(self_launch(args, sys.argv[1:], one_device))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks; refusing to report "
                         f"n_gpus for a job of a different size")
    if args.rendezvous_check:
        return rendezvous_check(args, rank, world)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (the product has no CPU path)")
    ndev = torch.cuda.device_count()
    if one_device:
        local_rank = 0
    elif ndev < world or local_rank >= ndev:
        raise SystemExit(f"bench.py: --gpus {args.gpus} needs {world} visible HIP devices, torch.cuda.device_count() = {ndev} "
                         f"(DZN_BENCH_ONE_DEVICE=1 rehearses the N-rank path on one device)")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    backend = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # "nccl" is RCCL on ROCm.  RCCL refuses two ranks on one device, so the one-device rehearsal stages through gloo.
        backend = os.environ.get("DZN_BENCH_BACKEND", "gloo" if one_device else "nccl")
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=dev)
        else:
            dist.init_process_group(backend=backend)
        if dist.get_world_size() != args.gpus:
            raise SystemExit(f"bench.py: process group has {dist.get_world_size()} ranks, --gpus {args.gpus}")

    if args.only_config1:
        print(json.dumps(config1_leg(args, dev)))
        return
    from diarizen_amd import _lib
    from diarizen_amd.configs import RESNET34, get_seg_config
    from diarizen_amd.dist import gather_windows
    from diarizen_amd.engine import Engine
    from diarizen_amd.inference import WindowRunner
    from testkit.synth import synth_recording_range
    from testkit.weights import emb_state_dict, seg_state_dict, turn_taking_state_dict   # seeded init (no checkpoints offline)

    cfg = get_seg_config(args.model)
    # the timed steps run on the workload the metric names: weights whose hard decisions change within a window, so the
    # clean-mask AND the fallback branch of prepare_masks, silent (window, speaker) pairs and the trunk-skip path all
    # occur — same kernels and flops as plain seeded weights (which put every frame in one powerset class)
    sd = turn_taking_state_dict(cfg, 0) if args.weights == "turn_taking" else seg_state_dict(cfg, 0)
    esd = emb_state_dict(0)
    sr = 16000
    window = int(args.window * sr)
    eng = Engine(cfg, sd, RESNET34, esd, max_batch=args.batch, max_samples=window,
                 precision=args.precision, device=dev)
    extra = tuple(Engine(cfg, sd, RESNET34, esd, max_batch=args.batch, max_samples=window, precision=args.precision, device=dev)
                  for _ in range(max(0, args.streams - 1)))
    runner = WindowRunner(eng, args.window, 0.1, args.batch, extra_engines=extra)
    if args.streams > 1:
        args.no_profile = True
    num_samples = int(args.minutes * 60 * sr)
    audio_s = num_samples / sr
    strong = args.scaling == "strong" and world > 1
    if strong:
        # ONE recording (seed 3407) for all ranks; this rank generates and uploads only the samples its windows touch
        c0, c1, s0, ns = shard_slice(num_samples, runner.window, runner.step, rank, world)
        wave_host = synth_recording_range(s0, ns, total=num_samples, seed=3407)
        n_windows = runner.num_windows(num_samples)
    else:
        wave_host = synth_recording(num_samples, seed=3407 + rank)
        n_windows = runner.num_windows(num_samples)
    wave = wave_host.to(dev)

    full = args.stage == "full"
    legs = extra_legs(args, world)
    # (r5) a step is the WHOLE pipeline of BASELINE configs[2] — "segmentation + embedding + AHC" — on a recording resident in
    # HBM: device hot path, results to the host, then the host stage (speaker counting, centroid-linkage AHC, constrained
    # assignment, reconstruction, Binarize, RTTM text: diarizen/pipelines/inference.py:137-185) through the product's
    # run_host_stage with its device backends.  Weak scaling: every rank owns a recording and runs its own host stage (the
    # all-gather to rank 0 stays in the step: it is the path's one exchange); strong: rank 0 runs it on the gathered windows.
    from diarizen_amd.clustering import AgglomerativeClustering
    from diarizen_amd.core import SlidingWindow
    from diarizen_amd.pipeline import run_host_stage
    clu = pipeline_conf(args, cfg)["clustering"]["args"]
    clustering = AgglomerativeClustering(metric="cosine", method="centroid", min_cluster_size=clu["min_cluster_size"],
                                         threshold=clu["ahc_threshold"])
    clustering.device = dev.index if dev.index is not None else 0
    chunks_sw = SlidingWindow(start=0.0, duration=args.window, step=0.1 * args.window)
    acc = {"on": False, "device_s": 0.0, "host_s": 0.0, "host_wait_s": 0.0, "speakers": 0, "rttm_lines": 0}
    last = {"seg": None, "emb": None, "tracks": None}       # the last timed step's results (--dump-outputs)

    def host(seg_t, emb_t):
        ann = run_host_stage(seg_t.numpy(), emb_t.numpy(), chunks=chunks_sw, clustering=clustering,
                             min_speakers=clu["min_speakers"], max_speakers=clu["max_speakers"], sess_name="bench", device=dev)
        rttm = ann.to_rttm()
        acc["speakers"], acc["rttm_lines"] = len(ann.labels()), len(rttm.splitlines())
        if acc["on"] and args.dump_outputs:      # host stages finish in step order: the last write is the last timed step's
            spk = {lab: i for i, lab in enumerate(ann.labels())}
            last["tracks"] = [(s.start, s.end, spk[lab]) for s, _, lab in ann.itertracks(yield_label=True)]
        return rttm

    def device_part():
        res = runner.run(wave, with_embeddings=full) if wave.numel() else None
        if not full:
            return res.segmentations.cpu(), None
        if world > 1:
            if strong:      # ranks hold different window counts: padded all-gather in window order (dist.py)
                S, L = eng.seg.max_speakers_per_chunk, runner.num_frames
                seg_l = res.segmentations if res is not None else torch.empty((0, L, S), device=dev, dtype=torch.uint8)
                emb_l = res.embeddings if res is not None else torch.empty((0, S, eng.emb.embed_dim), device=dev)
                seg_g, emb_g = gather_windows(seg_l, emb_l, expected_total=n_windows, to_host=rank == 0)
                return (seg_g, emb_g) if rank == 0 else (None, None)
            own = (res.segmentations.cpu(), res.embeddings.cpu())       # this rank's recording: its own host stage below
            # the path's one exchange (dist.py): ONE all_gather_into_tensor of the packed per-window results; every rank holds
            # n_windows of them, so the partition the gather verifies is the equal-block one; rank 0 takes the corpus to the host
            _ = gather_windows(res.segmentations, res.embeddings, expected_total=world * n_windows, to_host=rank == 0)
            return own
        return res.segmentations.cpu(), res.embeddings.cpu()

    # (r5) consecutive steps form a two-stage software pipeline, as DiariZenPipeline.diarize_many does over a
    # corpus: the host stage of step i runs in a worker thread WHILE the device stage of step i+1 executes (the host stage's
    # device work has its own high-priority stream and arena: csrc/linkage.hip, postprocess.DevicePost).  Every step's host
    # stage completes inside the timed region (drain() before the closing synchronise).  --no-overlap = the serial steps of the
    # first r5 runs; `serial_ms_per_step` reports them from extra steps either way.
    from concurrent.futures import ThreadPoolExecutor
    pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="dzn-host-stage") if full and not args.no_overlap else None
    pending = [None]

    def host_timed(seg_t, emb_t):
        t = time.perf_counter()
        host(seg_t, emb_t)
        if acc["on"]:
            acc["host_s"] += time.perf_counter() - t

    def drain():
        if pending[0] is not None:
            pending[0].result()
            pending[0] = None

    def step(serial=False):
        t_a = time.perf_counter()
        seg_t, emb_t = device_part()               # the .cpu() copies inside synchronise
        t_b = time.perf_counter()
        if full and seg_t is not None:
            if pool is None or serial:
                drain()
                host_timed(seg_t, emb_t)
            else:
                drain()                            # step i-1's host stage (ran beside this step's device stage)
                pending[0] = pool.submit(host_timed, seg_t, emb_t)
        if acc["on"]:
            acc["device_s"] += t_b - t_a
            acc["host_wait_s"] += time.perf_counter() - t_b
            last["seg"], last["emb"] = seg_t, emb_t

    for _ in range(args.warmup):
        step()
    drain()
    # the in-situ HIP-event profiler runs INSIDE the timed steps (two event records per launch on the launch stream;
    # measured cost 1 % of the step, reported as `unprofiled_ms_per_step` from one extra step below)
    if not args.no_profile:
        # one untimed profiled step sizes the event pool: the timed region must not create HIP events
        _lib.profile_enable(True)
        step()
        drain()
        launches = sum(p["launches"] for p in _lib.profile_collect())
        _lib.profile_reserve(2 * launches * args.steps + 1024)
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    skip0 = eng.embed_skip_stats() if full else (0, 0)        # device counters, read OUTSIDE the timed region (before / after)
    power = PowerSampler(device=dev) if rank == 0 and not args.no_power else None
    if power:
        power.start()
    acc["on"] = True
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    t_tail = time.perf_counter()
    drain()                                     # the last step's host stage: nothing left to hide it behind
    acc["host_wait_s"] += time.perf_counter() - t_tail
    torch.cuda.synchronize()
    dt_own = time.perf_counter() - t0           # this rank's own K steps (before it waits for the others)
    acc["on"] = False
    if power:
        power.stop()
    if dist is not None:
        dist.barrier()
    dt = time.perf_counter() - t0
    skip1 = eng.embed_skip_stats() if full else (0, 0)
    prof = [] if args.no_profile else _lib.profile_collect()
    _lib.profile_enable(False)
    per_rank_ms = [round(dt / args.steps * 1e3, 2)]
    if dist is not None:
        tdev = dev if backend == "nccl" else torch.device("cpu")
        tt = torch.tensor([dt_own], device=tdev, dtype=torch.float64)
        every = [torch.zeros_like(tt) for _ in range(world)]
        dist.all_gather(every, tt)
        per_rank_ms = [round(e.item() / args.steps * 1e3, 2) for e in every]
        tt = torch.tensor([dt, acc["device_s"]], device=tdev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt, dev_max_s = tt[0].item(), tt[1].item()
    else:
        dev_max_s = acc["device_s"]
    unprofiled_ms = None
    if "serial" in legs:
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(2):
            step(serial=True)                   # device stage, THEN host stage: the step of the first r5 runs, unprofiled
        torch.cuda.synchronize()
        unprofiled_ms = (time.perf_counter() - t1) * 1e3 / 2
    if pool is not None:
        pool.shutdown(wait=True)
    dumped = None
    if args.dump_outputs and rank == 0:
        dumped = dump_outputs(args.dump_outputs, last["seg"], last["emb"], last["tracks"] if full else None)

    strong_min = strong_minutes(args, world)
    strong_res = None
    if "strong" in legs and world > 1:          # collective: every rank takes part
        del eng, runner, wave
        torch.cuda.empty_cache()
        strong_res = strong_leg(args, dev, rank, world, strong_min)
        eng = None

    if rank == 0:
        ms_per_step = dt / args.steps * 1e3
        total_audio = audio_s if strong else world * audio_s
        value = total_audio * args.steps / dt
        device_value = total_audio * args.steps / dev_max_s if dev_max_s > 0 else None
        serial_ms = round(unprofiled_ms, 2) if unprofiled_ms else None
        serial_value = round(total_audio * 1e3 / unprofiled_ms, 2) if unprofiled_ms else None
        roofline = None
        kernels = []
        extra = {}
        if prof:
            tot_ms = sum(p["ms"] for p in prof)
            for p in sorted(prof, key=lambda p: -p["ms"]):
                e = {"kernel": p["name"], "launches": p["launches"], "ms_total": round(p["ms"], 3),
                     "share_of_profiled": round(p["ms"] / tot_ms, 4)}
                if p["flops"] > 0 and p["ms"] > 0:
                    e["tflops"] = round(p["flops"] / (p["ms"] * 1e-3) / 1e12, 2)
                if p["bytes"] > 0 and p["ms"] > 0:
                    e["gbs"] = round(p["bytes"] / (p["ms"] * 1e-3) / 1e9, 1)
                    e["alg_bytes_per_launch"] = int(p["bytes"] / p["launches"])
                # which roof the class sits under: algorithmic intensity against the ridge of ITS arithmetic (peak flops of the
                # class's MFMA mix / 8 TB/s); classes below the ridge are priced against HBM, the others against the matrix pipe
                if p["ms"] > 0 and (p["flops"] > 0 or p["bytes"] > 0):
                    pk = PEAK_TFLOPS[prec_of(p["name"], {"f16": "f32h", "bf16": "bf16"}.get(args.precision, args.precision))]
                    mfma_bound = p["flops"] > 0 and (p["bytes"] <= 0 or p["flops"] / p["bytes"] >= pk * 1e12 / (PEAK_HBM_GBS * 1e9))
                    e["bound"] = "mfma" if mfma_bound else "hbm"
                    e["frac_of_bound"] = round((e["tflops"] / pk) if mfma_bound else (e.get("gbs", 0.0) / PEAK_HBM_GBS), 4)
                kernels.append(e)
            top = max(prof, key=lambda p: p["ms"])
            traffic = pmc_table(args)
            if top["flops"] > 0:
                prec = prec_of(top["name"])
                ach = top["flops"] / (top["ms"] * 1e-3) / 1e12
                roofline = {"kernel": top["name"], "bound": "mfma", "achieved": round(ach, 2),
                            "peak": round(PEAK_TFLOPS[prec], 1), "unit": "TFLOP/s",
                            "frac": round(ach / PEAK_TFLOPS[prec], 4),
                            **other_roof(top, prec),
                            "traffic": pmc_lookup(traffic, top["name"], "hbm_bytes_per_launch"),
                            "traffic_source": f"{TRAFFIC_SOURCE} [{traffic.get('_file')}]" if traffic else None,
                            "rocprof_kernel_trace": rocprof_trace_name(args),
                            "launches": top["launches"],
                            "avg_launch_ms": round(top["ms"] / top["launches"], 4),
                            "alg_gflop_per_launch": round(top["flops"] / top["launches"] / 1e9, 3),
                            "alg_bytes_per_launch": int(top["bytes"] / top["launches"]) if top["bytes"] > 0 else None}
                if prec == "f32h":
                    roofline["note"] = ("achieved = algorithmic fp32 flops / s; every 16x16x32 block costs 3 fp16 MFMAs "
                                        "(hi*hi + hi*lo + lo*hi), so peak = fp16 dense peak 2500 / 3; executed MFMA rate = "
                                        "3 x achieved")
                    roofline["executed_tflops"] = round(3 * ach, 1)
                if prec == "mx":
                    roofline["note"] = ("achieved = algorithmic flops / s of the reduced contraction; every 32x32x64 block costs 4 fp16 MFMAs "
                                        "(hi*hi, 8 passes each) + 2 block-scaled fp8 MFMAs (the cross terms, 16 passes each) = 64 passes "
                                        "where plain fp16 needs 32, so peak = fp16 dense peak 2500 / 2; issue-bound micro-benchmark of the "
                                        "same mix: 1008 TFLOP/s (profiles/r5_mx_probe.txt)")
                if prec == "f32s":
                    roofline["note"] = ("achieved = algorithmic fp32 flops / s; every 16x16x32 block costs 6 bf16 "
                                        "MFMAs, so peak = bf16 dense peak 2500 / 6; executed MFMA rate = 6 x achieved")
                    roofline["executed_tflops"] = round(6 * ach, 1)
            else:
                ach = top["bytes"] / (top["ms"] * 1e-3) / 1e9
                roofline = {"kernel": top["name"], "bound": "hbm", "achieved": round(ach, 1),
                            "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(ach / PEAK_HBM_GBS, 4),
                            "traffic": pmc_lookup(traffic, top["name"], "hbm_bytes_per_launch"),
                            "launches": top["launches"],
                            "avg_launch_ms": round(top["ms"] / top["launches"], 4)}
            # north_star asks for two more figures: MFMA utilisation on the attention contractions and HBM GB/s on
            # the conv frontend.  Rates are live (HIP events of this run); MfmaUtil / PMC bytes come from the
            # committed rocprofv3 --pmc passes of the same command (profiles/, scripts/final_measure_r3.sh).
            for key, names in (("attention", ("attention_relpos_f32s", "attention_relpos_f32h", "attention_relpos_f32")),
                               ("conv_frontend", ("conv0_ln_gelu", "conv01_fused"))):
                p = next((p for p in prof if p["name"] in names), None)
                if p is None:
                    continue
                e = {"kernel": p["name"], "avg_launch_ms": round(p["ms"] / p["launches"], 4)}
                if p["flops"] > 0:
                    e["tflops"] = round(p["flops"] / (p["ms"] * 1e-3) / 1e12, 2)
                if p["bytes"] > 0:
                    e["alg_bytes_per_launch"] = int(p["bytes"] / p["launches"])
                    e["gbs"] = round(p["bytes"] / (p["ms"] * 1e-3) / 1e9, 1)
                    e["frac_of_hbm_peak"] = round(e["gbs"] / PEAK_HBM_GBS, 4)
                e["pmc_hbm_bytes_per_launch"] = pmc_lookup(traffic, p["name"], "hbm_bytes_per_launch")
                e["pmc_mfma_util_pct"] = pmc_lookup(traffic, p["name"], "mfma_util_pct")
                if p["name"] == "conv01_fused":
                    e["note"] = ("conv0 + LayerNorm + GELU + conv1 fused (frontend_fused.hip; r6: producer / consumer wavefronts in persistent workgroups, conv01_ws_kernel): conv0's 13.2 GB / launch of "
                                 "activations never reach HBM (was conv0_ln_gelu: 13.2 GB written at 2.7-2.8 TB/s = 0.34 of "
                                 "peak, then re-read by conv1); the kernel is MFMA/VALU-bound, its HBM traffic is the "
                                 "waveform in + conv1's raw output out (alg_bytes_per_launch; PMC beside it)")
                    e.pop("frac_of_hbm_peak", None)
                extra[key] = e
            extra["kernel_ms_per_step"] = round(tot_ms / args.steps, 2)
            extra["non_kernel_frac"] = round(1.0 - tot_ms / args.steps / ms_per_step, 4)
        out = {
            "metric": "audio-seconds/s (RTF) for wavlm-large-s80 pipeline, 16 kHz mono",
            "value": round(value, 2), "unit": "audio-seconds/s", "rtf": round(1.0 / value, 6),
            "n_gpus": world, "rccl_ranks": (world if backend == "nccl" else 0) if world > 1 else 1,
            "collective_backend": ("rccl (torch.distributed 'nccl' on ROCm)" if backend == "nccl" else backend) if world > 1 else None,
            "per_rank_ms_per_step": per_rank_ms,
            "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 2), "higher_is_better": True,
            "scaling": "strong" if strong else "weak",
            "vs_baseline": None, "dtype": DTYPE_NOTE[args.precision], "data": "synthetic",
            "config": {"workload": (f"{args.model} FULL pipeline (BASELINE configs[2]: segmentation + masks + ResNet34 embeddings on the "
                                    f"device, results to the host, then speaker counting + centroid-linkage AHC + constrained "
                                    f"assignment + reconstruction + Binarize + RTTM)" if full else f"{args.model} segmentation only") +
                                   f", {args.minutes:g} min synthetic 16 kHz mono {'sharded over the ranks' if strong else 'per GPU'}, "
                                   f"recording resident in HBM, window {args.window:g} s, step {0.1 * args.window:g} s, "
                                   f"{n_windows} windows, batch {args.batch}; host stage of step i {'pipelined beside the device stage of step i+1' if pool is not None else 'serially behind its device stage'}; `device_value` = the device hot path alone "
                                   f"(r1-r4's `value`), `e2e` = the same through DiariZenPipeline incl. the host -> HBM upload",
                       "cpu_baseline_kind": None,
                       # audit keys, inside `config` because the driver keeps this object whole:
                       "device_value": round(device_value, 2) if device_value else None,
                       "serial_value": serial_value,
                       "emb_windows_per_step": (skip1[0] - skip0[0]) // max(args.steps, 1) if full else None,
                       "emb_trunk_skipped_per_step": (skip1[1] - skip0[1]) // max(args.steps, 1) if full else None,
                       "emb_note": "windows handed to dzn_embed_forward per step / windows whose ResNet34 trunk was skipped because no "
                                   "local speaker was active (dzn_embed_skip_stats, device counters read before and after the timed "
                                   "region): 36.18 of the 104.9 algorithmic GFLOP per window are executed only for the others",
                       "windows_per_step": n_windows, "batch": args.batch, "launches": batches_note(n_windows, args.batch),
                       "weights": ("seeded turn-taking weights (testkit/weights.py: random init + Hann depthwise taps + calibrated "
                                   "classifier -> many powerset classes, both mask branches; no checkpoints offline)"
                                   if args.weights == "turn_taking" else "seeded random init (no checkpoints offline)")},
            "windows_per_s": round((1 if strong else world) * n_windows * args.steps / dt, 1),
            "device_value": round(device_value, 2) if device_value else None,
            "step_breakdown": {"device_ms": round(acc["device_s"] / args.steps * 1e3, 2), "host_ms": round(acc["host_s"] / args.steps * 1e3, 2),
                               "host_exposed_ms": round(acc["host_wait_s"] / args.steps * 1e3, 2),
                               "host_stage_overlapped": pool is not None,
                               "speakers": acc["speakers"], "rttm_lines": acc["rttm_lines"],
                               "note": "rank 0's own steps: device = hot path + D2H of the u8 decisions / f32 embeddings (+ the all-gather "
                                       "at N > 1), host = run_host_stage (device linkage / cdist / aggregations from their size "
                                       "thresholds up) + RTTM text, as busy time of the worker thread; host_exposed = what the stepping "
                                       "thread waited for it (step i's host stage runs beside step i+1's device stage; the last one of "
                                       "the K is drained inside the timed region)"},
            "unprofiled_ms_per_step": serial_ms,
            "serial_ms_per_step": serial_ms,
            "serial_value": serial_value,
            "roofline": roofline,
            "power": power.result() if power else None,
            "roofline_extra": extra,
            "parity": PARITY_NOTE,
            "kernels": kernels,
        }
        if dumped is not None:
            out["dumped_outputs"] = {"dir": str(args.dump_outputs), "shapes": dumped}
        if "other_modes" in legs:
            # the same workload in the other fp32 modes (strict parity tests run in all three)
            alt = {}
            for prec in ("f32s", "f32h", "f32"):
                if prec == args.precision:
                    continue
                dt2 = run_mode(cfg, sd, esd, wave, args, window, prec, full, dev)
                alt[prec] = {"value": round(audio_s / dt2, 2), "unit": "audio-seconds/s", "scope": "device hot path (compare with device_value)",
                             "ms_per_step": round(dt2 * 1e3, 2), "steps": ALT_STEPS, "dtype": DTYPE_NOTE[prec]}
            out["other_fp32_modes"] = alt
            out["fp32_mfma_mode"] = alt["f32"]
            # REDUCED precision (BASELINE configs[4] "fp16"): reported beside the headline, never as `value`
            dt2, prof16 = run_mode(cfg, sd, esd, wave, args, window, "f16", full, dev, profile=not args.no_profile)
            red = {"value": round(audio_s / dt2, 2), "unit": "audio-seconds/s", "scope": "device hot path (compare with device_value)",
                   "ms_per_step": round(dt2 * 1e3, 2), "steps": ALT_STEPS, "dtype": DTYPE_NOTE["f16"], "parity": reduced_parity()}
            if prof16:
                tot16 = sum(p["ms"] for p in prof16)
                top16 = max((p for p in prof16 if "gemm_mx" in p["name"]), key=lambda p: p["ms"], default=None)
                if top16 is not None and top16["ms"] > 0:
                    ach16 = top16["flops"] / (top16["ms"] * 1e-3) / 1e12
                    red["roofline"] = {"kernel": top16["name"], "bound": "mfma", "achieved": round(ach16, 2),
                                       "peak": PEAK_TFLOPS["mx"], "unit": "TFLOP/s", "frac": round(ach16 / PEAK_TFLOPS["mx"], 4),
                                       **other_roof(top16, "mx"),
                                       "share_of_profiled": round(top16["ms"] / tot16, 4), "launches": top16["launches"],
                                       "alg_bytes_per_launch": int(top16["bytes"] / top16["launches"]) if top16["bytes"] > 0 else None,
                                       "pmc_mfma_util_pct": pmc_lookup(pmc_table(args, "f16"), top16["name"], "mfma_util_pct"),
                                       "traffic": pmc_lookup(pmc_table(args, "f16"), top16["name"], "hbm_bytes_per_launch"),
                                       "avg_launch_ms": round(top16["ms"] / top16["launches"], 4),
                                       "note": "peak = the mix actually issued: per 32x32x64 block 4 fp16 MFMAs (8 passes) + 2 block-scaled "
                                               "fp8 MFMAs (16 passes) = 64 passes = fp16 dense peak / 2; the same mix issue-bound in a "
                                               "micro-benchmark: 1008 TFLOP/s (profiles/r5_mx_probe.txt)"}
                red["kernels"] = [{"kernel": p["name"], "ms_total": round(p["ms"], 2), "share_of_profiled": round(p["ms"] / tot16, 4),
                                   **({"tflops": round(p["flops"] / (p["ms"] * 1e-3) / 1e12, 1)} if p["flops"] > 0 and p["ms"] > 0 else {})}
                                  for p in sorted(prof16, key=lambda p: -p["ms"])[:8]]
            out["reduced_precision_mode"] = {"f16": red}
        if "two_streams" in legs:
            # the same steps with consecutive batches alternating over TWO engine handles / HIP streams (what DiariZenPipeline
            # does by default, num_streams = 2): reported beside the headline, whose steps stay on one stream because the
            # per-kernel event timing behind `roofline` is only meaningful there
            e2 = Engine(cfg, sd, RESNET34, esd, max_batch=args.batch, max_samples=window, precision=args.precision, device=dev)
            r2 = WindowRunner(eng, args.window, 0.1, args.batch, extra_engines=(e2,))     # the headline's handle + one more

            def one2():
                res = r2.run(wave, with_embeddings=full)
                _ = (res.segmentations.cpu(), res.embeddings.cpu()) if full else res.segmentations.cpu()
            one2()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            for _ in range(ALT_STEPS):
                one2()
            torch.cuda.synchronize()
            dt2 = (time.perf_counter() - t2) / ALT_STEPS
            e2.close()
            out["two_streams"] = {"value": round(audio_s / dt2, 2), "unit": "audio-seconds/s", "ms_per_step": round(dt2 * 1e3, 2),
                                  "steps": ALT_STEPS, "note": "consecutive batches alternate over two engine handles on two HIP "
                                  "streams (inference.WindowRunner extra_engines; the pipeline's default): same results bit "
                                  "for bit, independent batches overlap on the device; unprofiled"}
        if "e2e" in legs:
            eng = None
            torch.cuda.empty_cache()
            out["e2e"] = e2e_leg(args, dev, wave_host, sd, esd)
        if "strong" in legs and world == 1:     # one GPU: the same leg as the N > 1 runs, for the curve
            eng = None
            torch.cuda.empty_cache()
            strong_res = strong_leg(args, dev, rank, world, strong_min)
        if strong_res is not None:
            out["strong_scaling_e2e"] = strong_res
        if "config1" in legs:
            eng = runner = None
            import gc
            gc.collect()
            torch.cuda.empty_cache()
            out["config1"] = config1_leg(args, dev)
        if "cpu_baseline" in legs:
            out["cpu_baseline"] = cpu_baseline(cfg, sd, esd, window, 0.1 * args.window, clustering_args=clu)
            out["config"]["cpu_baseline_kind"] = out["cpu_baseline"]["kind"]
        # first-class companions of `value`, right behind it: the end-to-end rate (configs[2] as worded: upload + device
        # + host AHC, mean of --e2e-steps passes) and the same steps on the fp32 MFMA instruction (strict IEEE fp32 operands)
        head = {k: out.pop(k) for k in ("metric", "value", "unit", "rtf")}
        head["device_value"] = out.pop("device_value", None)
        head["e2e_value"] = out.get("e2e", {}).get("audio_seconds_per_s")
        head["fp32_mfma_value"] = out.get("fp32_mfma_mode", {}).get("value")
        print(json.dumps({**head, **out}))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
