# kernel trace + stats of bench.py (graph mode): bash tools/prof_step.sh <output dir>
O=$(realpath -m "${1:?usage: bash tools/prof_step.sh <output dir>}")
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
rocprofv3 --kernel-trace --stats -d $O --output-format csv -- python3 $R/bench.py --full --steps 10 --warmup 3 --cpu-baseline 0 > $O.json 2> $O.err
ls $O/*/ | head
