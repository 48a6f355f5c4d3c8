"""worker for tests/test_shortcut_fusion_gpu.py: DZN_NO_SHORTCUT_FUSION is read once, at dzn_create, so each form of the
down-sampling blocks gets an engine in a process of its own.  Embeds 3 windows of 2 s (the middle one silent) with the seeded
ResNet weights, replays the same forward from a HIP graph, and leaves the embeddings plus the kernel shapes the forward
launched in the file named on the command line."""
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
os.environ["DZN_PROFILE_SHAPES"] = "1"
import numpy as np
import torch

from diarizen_amd import _lib
from diarizen_amd.configs import RESNET34, get_seg_config
from diarizen_amd.engine import Engine
from oracle import seg_model
from oracle.gen_golden import synth_wave
from testkit.weights import emb_state_dict

out_path = sys.argv[1]
dev = torch.device("cuda:0")
cfg = get_seg_config("tiny_ln")
B, N, L = 3, 32000, 99
eng = Engine(cfg, seg_model.seg_state_dict(cfg, 0), RESNET34, emb_state_dict(0), max_batch=B, max_samples=N,
             precision="f32h", device=dev)
wave = synth_wave(B, N, 29).to(dev)
r = np.random.default_rng(5)
masks = torch.from_numpy((r.random((B, 4, L)) < 0.5).astype(np.float32))
masks[1] = 0.0                                       # the silent window sits in the middle of the batch
masks = masks.to(dev)
eng.embed(synth_wave(B, N, 30).to(dev), torch.ones_like(masks))   # every image buffer holds another batch's data
eager = eng.embed(wave, masks).clone()
torch.cuda.synchronize()
g = torch.cuda.CUDAGraph()
side = torch.cuda.Stream(device=dev)
side.wait_stream(torch.cuda.current_stream(dev))
with torch.cuda.stream(side):
    with torch.cuda.graph(g, stream=side):
        captured = eng.embed(wave, masks)
torch.cuda.synchronize()
captured.zero_()
g.replay()
torch.cuda.synchronize()
replay_equal = bool(torch.equal(eager, captured))
_lib.profile_enable(True)
eng.embed(wave, masks)
torch.cuda.synchronize()
names = [e["name"] for e in _lib.profile_collect()]
_lib.profile_enable(False)
eng.close()
torch.save({"emb": eager.cpu(), "replay_equal": replay_equal, "kernels": names}, out_path)
print("SHORTCUT_WORKER_OK")
