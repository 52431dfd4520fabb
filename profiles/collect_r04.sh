#!/bin/bash
# Everything the round-4 docs quote, collected on a GPU box from the build of this commit (run from the repo root), in
# parts that each finish within a few minutes and write only small summaries:
#   profiles/collect_r04.sh tests|bench|small|prof|train|pmc|pmctrain|bf16|sweep      -> gpurun_out/r04_*   (copy the summaries into profiles/)
o=gpurun_out
part=${1:-all}
want() { [ "$part" = all ] || [ "$part" = "$1" ]; }
if want tests; then
  python -m pytest tests -m gpu -q -p no:cacheprovider 2>&1 | grep -E "^[0-9]+ passed|^[0-9]+ failed| passed| failed|^ERROR|^FAILED" | tail -8 > $o/r04_gputest.log
  cat $o/r04_gputest.log
fi
if want bench; then
  python bench.py --full > $o/r04_bench_n1.json 2> $o/r04_bench_n1.err
  { python bench.py --full --dtype split --no-cpu-baseline; python bench.py --full --dtype bf16 --no-cpu-baseline;
    python bench.py --full --shape config5 --no-cpu-baseline --steps 5; python bench.py --full --shape config5 --dtype bf16 --no-cpu-baseline --steps 5;
    python bench.py --full --shape config5 --dtype split --no-cpu-baseline --steps 5; } 2>/dev/null | grep '^{' > $o/r04_modes_bench.jsonl
  { python bench.py --mode train --steps 4 --warmup 4; python bench.py --mode train --dtype bf16 --steps 4 --warmup 4;
    python bench.py --mode train --dtype split --steps 4 --warmup 4; } 2>/dev/null | grep '^{' > $o/r04_train_bench.jsonl
fi
if want small; then
  python profiles/small_batch.py 2>/dev/null | grep '^{' > $o/r04_other_configs.jsonl
  python profiles/small_sweep.py 1 2 3 4 6 8 16 32 2>/dev/null | grep '^{' > $o/r04_small_sweep.jsonl
  python profiles/eval_loop_probe.py 1 2 4 6 2>/dev/null | grep '^{' > $o/r04_eval_loop.jsonl
  { python profiles/multi_stream_probe.py 1 1 2 4 8; python profiles/multi_stream_probe.py 4 1 2 4; } 2>/dev/null | grep '^{' > $o/r04_multi_stream.jsonl
  profiles/prof.sh $o/r04_b1_kernel_stats.csv python $PWD/profiles/b1_profile.py 1 50
fi
if want prof; then
  profiles/prof.sh $o/r04_kernel_stats.csv python $PWD/bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-train-extra --no-small-extra --no-split-extra
fi
if want train; then
  python profiles/train_step.py 16 64 256 2>/dev/null | grep '^{' > $o/r04_train_step.jsonl
  PROF_TRACE="$PWD/$o/r04_train_trace.csv 1500" profiles/prof.sh $o/r04_train_kernel_stats.csv python $PWD/bench.py --mode train --steps 3 --warmup 1
  python profiles/gemm_probe.py 2>/dev/null | grep '^{' > $o/r04_gemm_probe.jsonl
  profiles/prof.sh $o/r04_train_bf16_kernel_stats.csv python $PWD/bench.py --mode train --dtype bf16 --steps 3 --warmup 1
  profiles/prof.sh $o/r04_train_split_kernel_stats.csv python $PWD/bench.py --mode train --dtype split --steps 3 --warmup 1
fi
if want pmctrain; then   # counters for config 3 (MFMA busy, FETCH / WRITE per training kernel)
  profiles/pmc.sh /tmp/pmc_r04t --mode train > /dev/null 2>&1
  python profiles/summarize_pmc.py /tmp/pmc_r04t $o/r04_train_pmc_summary.csv r04train > /dev/null
  rm -rf /tmp/pmc_r04t
fi
if want bf16; then
  profiles/prof.sh $o/r04_bf16_kernel_stats.csv python $PWD/bench.py --full --dtype bf16 --steps 5 --warmup 2 --no-cpu-baseline
  profiles/prof.sh $o/r04_split_kernel_stats.csv python $PWD/bench.py --full --dtype split --steps 5 --warmup 2 --no-cpu-baseline
  profiles/pmc.sh /tmp/pmc_r04b --dtype bf16 > /dev/null 2>&1
  python profiles/summarize_pmc.py /tmp/pmc_r04b $o/r04_bf16_pmc_summary.csv r04bf16 > /dev/null
  rm -rf /tmp/pmc_r04b
fi
if want pmc; then
  profiles/pmc.sh /tmp/pmc_r04 > /dev/null 2>&1
  python profiles/summarize_pmc.py /tmp/pmc_r04 $o/r04_pmc_summary.csv r04 > /dev/null
  rm -rf /tmp/pmc_r04
  # counters for config 2 (B = 64) as well
  profiles/pmc.sh /tmp/pmc_r04b --shape config2 > /dev/null 2>&1
  python profiles/summarize_pmc.py /tmp/pmc_r04b $o/r04_pmc_summary_b64.csv r04b64 > /dev/null
  rm -rf /tmp/pmc_r04b $o/r04b64_trunk_hbm_bytes.json
  profiles/pmc.sh /tmp/pmc_r04s --dtype split > /dev/null 2>&1
  python profiles/summarize_pmc.py /tmp/pmc_r04s $o/r04_split_pmc_summary.csv r04split > /dev/null
  rm -rf /tmp/pmc_r04s
fi
if want sweep; then
  python profiles/parity_sweep.py 2>/dev/null | grep '^{' > $o/r04_parity_sweep.jsonl
  python bench.py --full --shape config2 --no-cpu-baseline --no-train-extra --no-small-extra --no-split-extra 2>/dev/null | grep '^{' > $o/r04_config2_bench.json
fi
