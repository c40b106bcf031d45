#!/usr/bin/env bash
# ONE script for everything that is run on the GPU box through gpurun (it replaces round 5's r05_*.sh / collect_r0*.sh one-offs):
#
#   gpurun --timeout 900 -- 'tools/gpu_run.sh <out-subdir> <step> [<step> ...]'
#
# Steps run in the order given; their logs go to gpurun_out/<out-subdir>/ and a short digest of each to stdout (what gpurun
# shows).  A step is a word, or word:argument[:argument]:
#
#   suite[:<pytest args>]    pytest tests -m gpu -x
#   tests:<file>[,<file>]    the named test files only (tests/ is implied), e.g. tests:test_gpu_plugin_cxx.py
#   bench[:<bench.py args>]  the default bench line -> bench.json (+ one-line digest)
#   benchn:<N>[:<bench.py args>]  bench.py --gpus N as the driver launches it, but on ONE GPU: N ranks over gloo sharing device 0
#                            (PM_BENCH_BACKEND=gloo PM_BENCH_SHARE_DEVICE=1) — the plumbing of the N > 1 line, not its numbers
#   timing[:<rounds>]        cold matches of configs[1] and [2] (tools/variant_bench.py) + 8 churn ticks, <rounds> times (2)
#   variants:<a>,<b>         the same timings for prebuilt protocol_amd/variants/libpm_engine_<name>.so (tools/build_variants.py),
#                            product library first and last
#   env:"VAR=val VAR2=val"   the same timings of the product library under environment knobs
#   kstat[:<variant>,...]    rocprofv3 --kernel-trace --stats of 20 matches -> average duration of the carve's kernels
#   anatomy                  streaming carve taken apart with the prebuilt PM_CARVE_PROF library (tools/stream_prof.py), 10k / 100k
#   timeline                 product-like timelines (prebuilt PM_ROW_REC library, tools/stream_trace.py): 10k, 100k, churn
#   pipeline[:<args>]        a ticket's way through the streaming carve on one clock (prebuilt PM_ROW_REC library, tools/pipeline_probe.py)
#   host                     PM_TRACE_HOST marks of a cold match and of churn ticks + the rocprofv3 kernel timeline of a match
#   profiles:<rNN>           tools/collect_profiles.py <rNN>: kernel statistics, PMC passes, bench line -> gpurun_out/<rNN>/
#   fuzz[:<swarms>[:<seed>[:<kind>,<kind>]]]  tools/parity_fuzz.py (engine against oracle on random swarms; all kinds unless named)
#   liveness[:<args>]        tools/liveness_probe.py [W] [--bench DIR]: pm_liveness_sweep at W rows (100000), reporting and applying
#                            -> r18_liveness.txt (copy it to profiles/)
#   discovery[:<args>]       tools/discovery_probe.py [W] [--bench DIR]: pm_discovery_sync at W rows (100000), three shapes, beside each
#                            the sequential D x W loop on one host thread -> r19_discovery.txt (copy it to profiles/)
#   metrics[:<args>]         tools/metrics_probe.py [W] [E] [--bench DIR]: pm_metrics_ingest / _totals / _rows at W rows (100000) x E
#                            series a row (8), beside each the same call as an unordered_map per node on one host thread
#                            -> r20_metrics.txt (copy it to profiles/)
#   rollout[:<args>]         tools/rollout_probe.py [W] [--bench DIR]: pm_rollout_ingest and the four reads at W rows (100000) over the
#                            groups of a real tick, beside each the same work as a loop on one host thread
#                            -> r26_rollout.txt (copy it to profiles/)
#   directory[:<args>]       tools/directory_probe.py [W ...] [--bench DIR]: pm_directory at 10,000 and 100,000 rows — the counters, a
#                            first and a middle page by row and by address, the full list — beside each what a host does today
#                            (three full-table reads, a stable sort, the join) -> r27_directory.txt (copy it to profiles/)
#   groupdir[:<args>]        tools/groupdir_probe.py [W ...] [--bench DIR]: pm_group_directory at 10,000 and 100,000 rows — the counters,
#                            a first and a middle page in each order, the degraded filter, the full list — beside each what a host
#                            does today (pm_get_groups + pm_liveness_get + pm_rollout_groups, the join, a sort of id texts)
#                            -> r28_group_directory.txt (copy it to profiles/)
#   taskdir[:<args>]         tools/taskdir_probe.py [T:W ...] [--bench DIR]: pm_task_directory at 100,000 tasks over 10,000 workers and
#                            1,000,000 over 100,000 — the counters, a first and a middle page in each order, the starved filter, the
#                            full list — beside each what a host does today (pm_task_report + pm_rollout_tasks whole, a hash-map
#                            join on ids, classification, filter, sort) -> r29_task_directory.txt (copy it to profiles/)
#   addresses[:<args>]       tools/address_probe.py [W ...] [--bench DIR]: the address book at 10,000, 100,000 and 1,000,000 rows with
#                            1 % appended a step — pm_addresses_set, pm_addresses_rank on both sort paths, a page of texts, the invite
#                            digests — beside the set + rank pair what the plugin does today (an EIP-55 text per new address, the
#                            sorted insert, the re-rank, pm_set_addr_ranks) -> r30_address_book.txt (copy it to profiles/)
#   gate[:<args>]            tools/gate_probe.py [n ...] [--bench DIR]: pm_ecrecover_many and pm_verify_requests at 1,000, 10,000 and
#                            100,000 requests over a book of 100,000 rows, the address index cold and warm, beside pm_host_ecrecover
#                            on one host thread -> r32_request_gate.txt (copy it to profiles/)
#   admission[:<args>]       tools/admission_probe.py [n ...] [--bench DIR]: pm_admit_requests beside pm_verify_requests at 1,000 and 10,000
#                            requests over standing nonce sets of 0, 100,000 and 1,000,000 entries, and pm_liveness_sweep_beats(NULL)
#                            beside pm_liveness_sweep at W = 100,000 -> r33_admission.txt (copy it to profiles/)
#   py:<script and args>     python tools/<script and args> (anything else)
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
ROOT=$PWD
sub=${1:?usage: tools/gpu_run.sh <out-subdir> <step>...}; shift
out=$ROOT/gpurun_out/$sub
mkdir -p "$out"
export TMPDIR=/tmp
n=0

timings() {  # $1 = log, $2 = rounds of configs[1], $3 = rounds of configs[2]; PM_EXP_LIB / env come from the caller
  timeout 120 python tools/variant_bench.py 1 "$2" >> "$1" 2>&1
  timeout 120 python tools/variant_bench.py 2 "$3" >> "$1" 2>&1
  timeout 120 python tools/churn_probe.py 8 2>&1 | grep "^tick" | awk '{s+=$3; n++} END {if (n) printf "churn ticks mean %.3f ms over %d\n", s/n, n}' >> "$1"
}
digest() { grep -v "^  " "$1" | sed 's/defines .*: carve/carve/; s/, groups.*//'; }

for step in "$@"; do
  n=$((n+1))
  name=${step%%:*}; arg=""; [ "$step" != "$name" ] && arg=${step#*:}
  echo "##### [$n] $step"
  case $name in
    suite)
      timeout 900 python -m pytest tests -m gpu -q -p no:cacheprovider -rfE -x $arg > "$out/${n}_suite.log" 2>&1
      echo "suite rc=$?" | tee -a "$out/${n}_suite.log"; tail -4 "$out/${n}_suite.log" ;;
    tests)
      files=$(echo "$arg" | tr ',' '\n' | sed 's#^#tests/#' | tr '\n' ' ')
      timeout 900 python -m pytest $files -m gpu -q -p no:cacheprovider -rfE -x > "$out/${n}_tests.log" 2>&1
      echo "tests rc=$?" | tee -a "$out/${n}_tests.log"; tail -6 "$out/${n}_tests.log" ;;
    bench)
      timeout 600 python bench.py $arg > "$out/bench.json" 2> "$out/bench.err"; echo "bench rc=$?"
      python - "$out/bench.json" <<'PY'
import json, sys
try:
    d = json.loads([l for l in open(sys.argv[1]) if l.startswith("{")][-1])
    print("ms_per_step", d["ms_per_step"], "roofline", d.get("roofline"))
    for k in ("churn", "configs2", "merge", "dist"):
        if k in d:
            print(" ", k, {a: b for a, b in d[k].items() if not isinstance(b, (list, dict))})
except Exception as ex:
    print("no bench line:", ex)
PY
      ;;
    benchn)
      nr=${arg%%:*}; rest=""; [ "$arg" != "$nr" ] && rest=${arg#*:}
      PM_BENCH_BACKEND=gloo PM_BENCH_SHARE_DEVICE=1 timeout 900 python -m torch.distributed.run --nnodes=1 --nproc-per-node "$nr" \
        --master-addr 127.0.0.1 --master-port 29511 bench.py --gpus "$nr" --steps 5 --warmup 2 $rest > "$out/bench_n${nr}_gloo.json" 2> "$out/bench_n${nr}.err"
      echo "benchn rc=$?"; tail -3 "$out/bench_n${nr}.err"
      python - "$out/bench_n${nr}_gloo.json" <<'PY'
import json, sys
try:
    d = json.loads([l for l in open(sys.argv[1]) if l.startswith("{")][-1])
    print("n_gpus", d["n_gpus"], "scaling", d["scaling"], "ms_per_step", d["ms_per_step"], "value", d["value"], "ranks_seen", d.get("ranks_seen"))
    print("  one_pool_sharded", {a: b for a, b in d["dist"]["one_pool_sharded"].items() if not isinstance(b, (str, dict))})
except Exception as ex:
    print("no bench line:", ex)
PY
      ;;
    timing)
      for r in $(seq 1 "${arg:-2}"); do timings "$out/${n}_timing.log" 20 8; done
      digest "$out/${n}_timing.log" ;;
    variants)
      for v in "" $(echo "$arg" | tr ',' ' ') ""; do
        lib=""; [ -n "$v" ] && lib="protocol_amd/variants/libpm_engine_$v.so"
        echo "=== variant '${v:-product}'" >> "$out/${n}_variants.log"
        PM_EXP_LIB=$lib timings "$out/${n}_variants.log" 20 8
      done
      digest "$out/${n}_variants.log" ;;
    env)
      for v in "" "$arg" ""; do
        echo "=== env '${v:--}'" >> "$out/${n}_env.log"
        env $v bash -c "$(declare -f timings); timings '$out/${n}_env.log' 20 8"
      done
      digest "$out/${n}_env.log" ;;
    kstat)
      for v in $(echo "$arg" | tr ',' ' ') "product"; do
        lib=""; [ "$v" != "product" ] && lib="$ROOT/protocol_amd/variants/libpm_engine_$v.so"
        d="$out/tr_$v"
        (cd /tmp && PM_EXP_LIB=$lib timeout -k 5 200 rocprofv3 --kernel-trace --stats -d "$d" -o t -- python "$ROOT/tools/variant_bench.py" 1 20 > "$out/${n}_kstat_$v.log" 2>&1)
        echo "=== $v" >> "$out/${n}_kstat.txt"
        db=$(find "$d" -name "t_results.db" | head -1)
        python tools/rocpd_summary.py "$db" "$out/${n}_kstat_$v.csv" > /dev/null 2>&1
        grep "carve_stream_kernel\|carve_finish\|elig_place\|pair_sweep" "$out/${n}_kstat_$v.csv" >> "$out/${n}_kstat.txt"
        rm -rf "$d"
      done
      cat "$out/${n}_kstat.txt" ;;
    anatomy)
      P=protocol_amd/variants/libpm_engine_prof.so   # (tools/build_variants.py prof=PM_CARVE_PROF, built where there is no GPU)
      PM_PROF_LIB=$P PM_PROF_NO_BUILD=1 timeout 200 python tools/stream_prof.py 100000 10000 > "$out/stream_anatomy_10k.txt" 2>&1
      PM_PROF_LIB=$P PM_PROF_NO_BUILD=1 timeout 200 python tools/stream_prof.py 1000000 100000 > "$out/stream_anatomy_100k.txt" 2>&1
      grep "T=\|a row\|proposer rows\|chain anatomy\|compute\|networks\|bitmap sweeps" "$out/stream_anatomy_10k.txt" "$out/stream_anatomy_100k.txt" ;;
    timeline)
      L=protocol_amd/variants/libpm_engine_rowrec.so
      PM_PROF_LIB=$L PM_PROF_NO_BUILD=1 timeout 200 python tools/stream_trace.py 100000 10000 > "$out/stream_timeline_10k.txt" 2>&1
      PM_PROF_LIB=$L PM_PROF_NO_BUILD=1 timeout 200 python tools/stream_trace.py 1000000 100000 > "$out/stream_timeline_100k.txt" 2>&1
      PM_PROF_LIB=$L PM_PROF_NO_BUILD=1 timeout 200 python tools/stream_trace.py churn > "$out/stream_timeline_churn.txt" 2>&1
      head -30 "$out/stream_timeline_10k.txt"; grep "chain waits\|totals" "$out/stream_timeline_100k.txt"; head -12 "$out/stream_timeline_churn.txt" ;;
    pipeline)
      PM_EXP_LIB=protocol_amd/variants/libpm_engine_rowrec.so timeout 300 python tools/pipeline_probe.py $arg > "$out/${n}_pipeline.txt" 2>&1
      echo "pipeline rc=$?"; head -150 "$out/${n}_pipeline.txt" | cut -c1-200 ;;
    host)
      PM_TRACE_HOST=1 timeout 120 python tools/host_trace.py 1 2>&1 | tail -16 > "$out/host_marks_match.txt"
      PM_TRACE_HOST=1 timeout 120 python tools/churn_probe.py 8 2>&1 | tail -40 > "$out/host_marks_churn.txt"
      (cd /tmp && timeout -k 5 200 rocprofv3 --kernel-trace -d "$out/trace" -o t -- python "$ROOT/tools/host_trace.py" 1 > "$out/trace.log" 2>&1)
      db=$(find "$out/trace" -name "t_results.db" | head -1)
      python tools/tick_timeline.py "$db" --all > "$out/timeline.txt" 2>&1
      rm -rf "$out/trace"
      cat "$out/host_marks_match.txt" "$out/timeline.txt"; grep "^tick\|^cold" "$out/host_marks_churn.txt" ;;
    profiles)
      timeout 1200 python tools/collect_profiles.py "$arg" > "$out/${n}_collect.log" 2>&1; echo "collect rc=$?"
      tail -3 "$out/${n}_collect.log" | cut -c1-600 ;;
    fuzz)
      IFS=: read -r swarms seed kinds <<< "$arg"
      timeout 3000 python tools/parity_fuzz.py ${swarms:+--swarms $swarms} ${seed:+--seed $seed} ${kinds:+--kinds $kinds} > "$out/${n}_fuzz.txt" 2>&1; echo "fuzz rc=$?"
      tail -15 "$out/${n}_fuzz.txt" ;;
    liveness)
      timeout -k 10 300 python tools/liveness_probe.py $arg --out "$out/r18_liveness.txt" > "$out/${n}_liveness.log" 2>&1; echo "liveness rc=$?"
      tail -12 "$out/${n}_liveness.log" ;;
    discovery)
      timeout -k 10 300 python tools/discovery_probe.py $arg --out "$out/r19_discovery.txt" > "$out/${n}_discovery.log" 2>&1; echo "discovery rc=$?"
      tail -12 "$out/${n}_discovery.log" ;;
    metrics)
      timeout -k 10 300 python tools/metrics_probe.py $arg --out "$out/r20_metrics.txt" > "$out/${n}_metrics.log" 2>&1; echo "metrics rc=$?"
      tail -12 "$out/${n}_metrics.log" ;;
    rollout)
      timeout -k 10 300 python tools/rollout_probe.py $arg --out "$out/r26_rollout.txt" > "$out/${n}_rollout.log" 2>&1; echo "rollout rc=$?"
      tail -12 "$out/${n}_rollout.log" ;;
    directory)
      timeout -k 10 400 python tools/directory_probe.py $arg --out "$out/r27_directory.txt" > "$out/${n}_directory.log" 2>&1; echo "directory rc=$?"
      tail -20 "$out/${n}_directory.log" ;;
    groupdir)
      timeout -k 10 400 python tools/groupdir_probe.py $arg --out "$out/r28_group_directory.txt" > "$out/${n}_groupdir.log" 2>&1; echo "groupdir rc=$?"
      tail -24 "$out/${n}_groupdir.log" ;;
    taskdir)
      timeout -k 10 500 python tools/taskdir_probe.py $arg --out "$out/r29_task_directory.txt" > "$out/${n}_taskdir.log" 2>&1; echo "taskdir rc=$?"
      tail -40 "$out/${n}_taskdir.log" ;;
    addresses)
      timeout -k 10 600 python tools/address_probe.py $arg --out "$out/r30_address_book.txt" > "$out/${n}_addresses.log" 2>&1; echo "addresses rc=$?"
      tail -40 "$out/${n}_addresses.log" ;;
    gate)
      timeout -k 10 500 python tools/gate_probe.py $arg --out "$out/r32_request_gate.txt" > "$out/${n}_gate.log" 2>&1; echo "gate rc=$?"
      tail -30 "$out/${n}_gate.log" ;;
    admission)
      timeout -k 10 500 python tools/admission_probe.py $arg --out "$out/r33_admission.txt" > "$out/${n}_admission.log" 2>&1; echo "admission rc=$?"
      tail -30 "$out/${n}_admission.log" ;;
    py)
      timeout 1800 python tools/$arg > "$out/${n}_py.log" 2>&1; echo "py rc=$?"; tail -40 "$out/${n}_py.log" ;;
    *) echo "unknown step '$step'" ;;
  esac
done
