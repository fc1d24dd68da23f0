# Everything committed under profiles/ for one round, in one session on a GPU box (developer aid):
#   bash tools/collect_round_profiles.sh [DIR]        then copy DIR/* (default: round_out/) to
#   profiles/ under the round's names (rXX_* -> rNN_*)
set -x
export TMPDIR=/tmp
ROUND=${1:-round_out}
mkdir -p $ROUND
export OBE_PROF_ROOT=$ROUND          # the rocprofv3 databases go under DIR too, and are removed once summarised
( time python bench.py --steps 20 --warmup 5 --full > $ROUND/bench_c3.json 2> $ROUND/bench_c3.err ) 2> $ROUND/bench_c3.time
python bench.py --config c5 --steps 12 --warmup 3 --full > $ROUND/bench_c5.json 2>/dev/null
python bench.py --config c2 --steps 40 --warmup 5 --full > $ROUND/bench_c2.json 2>/dev/null
python bench.py --config c1 --steps 400 --warmup 20 --full > $ROUND/bench_c1.json 2>/dev/null
python tools/measure_demo_cycle.py > $ROUND/demo_cycle.txt 2>/dev/null
python tools/measure_update.py 3 > $ROUND/update_moments.txt 2>/dev/null
python tools/measure_update.py 10 >> $ROUND/update_moments.txt 2>/dev/null
python tools/shard_cycle.py c3 8 > $ROUND/shard_cycle_c4.txt 2>/dev/null
python tools/shard_cycle.py c5 8 > $ROUND/shard_cycle_c5.txt 2>/dev/null
python tools/spec_cycles.py c2 60 > $ROUND/spec_cycles_c2.txt 2>/dev/null
python tools/profile_host_split.py c1 2000 > $ROUND/host_split_c1.txt 2>/dev/null
python tools/profile_host_split.py c2 300 > $ROUND/host_split_c2.txt 2>/dev/null
bash tools/profile_rocprof.sh c3
bash tools/profile_rocprof.sh c5
bash tools/profile_rocprof.sh c2
bash tools/profile_sq.sh
for cfg in c3 c5 c2; do
  src=$ROUND/prof; [ $cfg != c3 ] && src=$ROUND/prof_$cfg
  ( for k in -9 -8 -7; do timeout 60 python tools/trace_cycle.py $src/trace/bench_results.db $k; echo; done ) > $ROUND/cycle_timeline_$cfg.txt 2>&1
done
# the rocpd databases are large: keep their summaries only
cp profiles/pmc_traffic.json $ROUND/ 2>/dev/null
OBE_PROFILE_DST=$ROUND python tools/summarize_profiles.py rXX c3 > /dev/null
OBE_PROFILE_DST=$ROUND python tools/summarize_profiles.py rXX c5 > /dev/null
OBE_PROFILE_DST=$ROUND python tools/summarize_profiles.py rXX c2 > /dev/null
rm -rf $ROUND/prof $ROUND/prof_c5 $ROUND/prof_c2 $ROUND/prof_sq
du -sh $ROUND
