"""Incremental-decoding tokens/s of the bench's LLaMA-7B workload (8 requests,
128 prompt + 128 decoded tokens, synthetic weights) with top-p sampling on
against off, through serve.generate on ONE model: Model.set_sampling switches
the tail between runs, the two settings alternate over R repeats after one
warm-up generate each (graph capture), and each timed window is G generates
ending in the serve call's own synchronisation.  LAYERS=n shortens the model
(rehearsals).  One JSON line, also written to bench_out/sampling_serve_bench.json.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("FFMI_BENCH_OUT") or os.path.join(ROOT, "bench_out")  # output directory
sys.path.insert(0, ROOT)
import flexflow_amd as fa  # noqa: E402
from bench import LLAMA_7B, make_prompts  # noqa: E402

B, P, D = 8, 128, 128
R = int(os.environ.get("R", 3))
G = int(os.environ.get("G", 3))
cfg = dict(LLAMA_7B)
if os.environ.get("LAYERS"):
    cfg["num_layers"] = int(os.environ["LAYERS"])
fa.set_device(0)
rm_kw = dict(max_requests_per_batch=B, max_tokens_per_batch=1024, max_sequence_length=512)
llm = fa.Model(cfg, "inc", max_requests=B, max_tokens=1024, max_seq_len=512, weight_seed=20250117)
prompts = make_prompts(B, P - 1, cfg["vocab_size"])
SETTINGS = {"greedy": None, "sampling": fa.GenerationConfig(do_sample=True)}


def generates(n):
    new = 0
    t0 = time.time()
    for _ in range(n):
        res = fa.generate(fa.RequestManager(**rm_kw), llm, prompts, max_length=P + D)
        new += sum(len(r.output_tokens) - len(r.input_tokens) for r in res)
    return new / (time.time() - t0)


rates = {k: [] for k in SETTINGS}
for name, gc in SETTINGS.items():  # warm-up: every graph of both tails
    llm.set_sampling(gc, seed=1)
    generates(1)
for _ in range(R):
    for name, gc in SETTINGS.items():
        llm.set_sampling(gc, seed=1)
        generates(1)  # (set_sampling drops the captured graphs)
        rates[name].append(round(generates(G), 1))
med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
out = dict(workload=f"llama7b_incr B={B} P={P} D={D} layers={cfg['num_layers']}",
           generates_per_window=G, tokens_per_s=rates, median=med,
           sampling_over_greedy=round(med["sampling"] / med["greedy"], 4))
print(json.dumps(out), flush=True)
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "sampling_serve_bench.json"), "w") as f:
    f.write(json.dumps(out) + "\n")
