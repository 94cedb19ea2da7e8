"""DV3-S graphed gradient-step time with a MultiDiscrete action space
(dummy_multidiscrete, MineDojo-like heads [19, 8, 12]), bf16, batch 16 x
sequence 64: run the real CLI loop up to the hipGraph capture, then time
replays of the captured step on its own batch between device synchronises.

    python probes/dv3_multidiscrete_step.py [--fused 0|1] [--replays N] [--rounds R]

--fused 0 forces the module-loop imagination + autograd losses
(algo.fused_imagination=False); on a tree without the ragged-head fast path
both settings take the module loop."""
import sys, os, tempfile, time, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import argparse
import inspect

import torch

from sheeprl_amd.algos.dreamer_v3 import dreamer_v3
from sheeprl_amd.cli import run

p = argparse.ArgumentParser()
p.add_argument("--fused", type=int, default=1)
p.add_argument("--replays", type=int, default=40)
p.add_argument("--rounds", type=int, default=5)
p.add_argument("--label", default="")
args = p.parse_args()

ROLLOUT_HEADS = []
_orig_rollout = dreamer_v3.imagine_rollout
def _counting_rollout(rssm, actor, *a, **k):
    ROLLOUT_HEADS.append(len(actor.mlp_heads))
    return _orig_rollout(rssm, actor, *a, **k)
dreamer_v3.imagine_rollout = _counting_rollout

RESULT = {}
_orig_capture = dreamer_v3._capture_train_step
_capture_sig = inspect.signature(_orig_capture)
def _timing_capture(*a, **k):
    graphed_step, graph_metrics = _orig_capture(*a, **k)
    assert graphed_step is not None, "graph capture failed: nothing to time"
    batch = _capture_sig.bind(*a, **k).arguments["example_batch"]
    for _ in range(10):
        graphed_step(batch)
    torch.cuda.synchronize()
    rounds = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        for _ in range(args.replays):
            graphed_step(batch)
        torch.cuda.synchronize()
        rounds.append((time.perf_counter() - t0) / args.replays * 1000)
    RESULT["ms_per_step_rounds"] = [round(x, 3) for x in rounds]
    RESULT["ms_per_step_median"] = round(sorted(rounds)[len(rounds) // 2], 3)
    return graphed_step, graph_metrics
dreamer_v3._capture_train_step = _timing_capture

tmp = tempfile.mkdtemp()
run(["exp=dreamer_v3_100k_ms_pacman", "env=dummy", "env.id=dummy_multidiscrete",
     "env.wrapper_kwargs.action_dims=[19,8,12]", "env.num_envs=1", "env.sync_env=True",
     "runtime.accelerator=cuda", "runtime.precision=bf16", "algo.replay_ratio=1",
     "algo.per_rank_batch_size=16", "algo.per_rank_sequence_length=64",
     f"algo.fused_imagination={bool(args.fused)}",
     "algo.learning_starts=128", "algo.total_steps=134", "buffer.size=4096", "buffer.checkpoint=False",
     "metric.log_level=0", "metric.disable_timer=True", "algo.run_test=False", "checkpoint.every=0",
     "checkpoint.save_last=False", f"root_dir={tmp}"])
assert RESULT, "the train step was never captured"
RESULT.update(label=args.label, fused_imagination=bool(args.fused),
              fast_rollout_calls=len(ROLLOUT_HEADS), rollout_heads=sorted(set(ROLLOUT_HEADS)))
print("RESULT " + json.dumps(RESULT))
