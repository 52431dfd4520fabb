#!/bin/bash
# Everything the round-2 docs quote, collected on a GPU box from the build of this commit (run from the repo root), in
# parts that each finish within a few minutes and write only small summaries:
#   profiles/collect_r03.sh tests|bench|small|prof|train|pmc|pmctrain|bf16      -> gpurun_out/r03_*   (copy the summaries into profiles/)
o=gpurun_out
part=${1:-all}
want() { [ "$part" = all ] || [ "$part" = "$1" ]; }
if want tests; then
  python -m pytest tests -m gpu -q -p no:cacheprovider 2>&1 | grep -E "passed|failed|error" | tail -5 > $o/r03_gputest.log
  cat $o/r03_gputest.log
fi
if want bench; then
  python bench.py --full > $o/r03_bench_n1.json 2> $o/r03_bench_n1.err
  { python bench.py --full --dtype split --no-cpu-baseline; python bench.py --full --dtype bf16 --no-cpu-baseline;
    python bench.py --full --shape config5 --no-cpu-baseline --steps 5; python bench.py --full --shape config5 --dtype bf16 --no-cpu-baseline --steps 5;
    python bench.py --full --shape config5 --dtype split --no-cpu-baseline --steps 5; } 2>/dev/null | grep '^{' > $o/r03_modes_bench.jsonl
  { python bench.py --mode train --steps 4 --warmup 4; python bench.py --mode train --dtype bf16 --steps 4 --warmup 4;
    python bench.py --mode train --dtype split --steps 4 --warmup 4; } 2>/dev/null | grep '^{' > $o/r03_train_bench.jsonl
fi
if want small; then
  python profiles/small_batch.py 2>/dev/null | grep '^{' > $o/r03_other_configs.jsonl
  python profiles/small_sweep.py 1 2 3 4 6 8 16 32 2>/dev/null | grep '^{' > $o/r03_small_sweep.jsonl
  python profiles/eval_loop_probe.py 1 2 4 6 2>/dev/null | grep '^{' > $o/r03_eval_loop.jsonl
  { python profiles/multi_stream_probe.py 1 1 2 4 8; python profiles/multi_stream_probe.py 4 1 2 4; } 2>/dev/null | grep '^{' > $o/r03_multi_stream.jsonl
  profiles/prof.sh $o/r03_b1_kernel_stats.csv python $PWD/profiles/b1_profile.py 1 50
fi
if want prof; then
  profiles/prof.sh $o/r03_kernel_stats.csv python $PWD/bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-train-extra --no-small-extra
fi
if want train; then
  python profiles/train_step.py 16 64 256 2>/dev/null | grep '^{' > $o/r03_train_step.jsonl
  PROF_TRACE="$PWD/$o/r03_train_trace.csv 1500" profiles/prof.sh $o/r03_train_kernel_stats.csv python $PWD/bench.py --mode train --steps 3 --warmup 1
  python profiles/gemm_probe.py 2>/dev/null | grep '^{' > $o/r03_gemm_probe.jsonl
fi
if want pmctrain; then   # counters for config 3 (MFMA busy, FETCH / WRITE per training kernel)
  profiles/pmc.sh /tmp/pmc_r03t --mode train > /dev/null 2>&1
  python profiles/summarize_pmc.py /tmp/pmc_r03t $o/r03_train_pmc_summary.csv r03train > /dev/null
  rm -rf /tmp/pmc_r03t
fi
if want bf16; then
  profiles/prof.sh $o/r03_bf16_kernel_stats.csv python $PWD/bench.py --full --dtype bf16 --steps 5 --warmup 2 --no-cpu-baseline
  profiles/prof.sh $o/r03_split_kernel_stats.csv python $PWD/bench.py --full --dtype split --steps 5 --warmup 2 --no-cpu-baseline
  profiles/pmc.sh /tmp/pmc_r03b --dtype bf16 > /dev/null 2>&1
  python profiles/summarize_pmc.py /tmp/pmc_r03b $o/r03_bf16_pmc_summary.csv r03bf16 > /dev/null
  rm -rf /tmp/pmc_r03b
fi
if want pmc; then
  profiles/pmc.sh /tmp/pmc_r03 > /dev/null 2>&1
  python profiles/summarize_pmc.py /tmp/pmc_r03 $o/r03_pmc_summary.csv r03 > /dev/null
  rm -rf /tmp/pmc_r03
fi
