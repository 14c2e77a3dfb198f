#!/bin/bash
# Evidence run for profiles/: full bench line, rocprofv3 kernel-trace stats of the graph-replayed step, inference bench.
cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
O=${1:?usage: tools/profile_round.sh OUT_DIR}; mkdir -p $O
timeout -k 10 400 python bench.py --full 2>$O/bench_full_err.txt | tail -1 > $O/bench_full.json || exit 1
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_graph -- python3 bench.py --steps 4 --warmup 2 --no-cpu-baseline --no-roofline > $O/prof_graph.log 2>&1 || exit 1
timeout -k 10 200 python bench.py --full --no-cpu-baseline --no-roofline --infer 2>/dev/null | tail -1 > $O/bench_infer.json || exit 1
ls $O/prof_graph/*/
