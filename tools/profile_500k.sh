R=$(cd "$(dirname "$0")/.." && pwd)
RES=${NIQKI_RESULTS:-$R/results}; mkdir -p $RES
cd /tmp; export TMPDIR=/tmp
rm -rf /tmp/kt5; timeout -k 10 800 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/kt5 -- python3 $R/bench.py --full --genomes 500000 --no-legs --steps 4 --warmup 1 > $RES/r05_500k_trace_$1.json 2> /tmp/kt5.log || { tail -5 /tmp/kt5.log; exit 1; }
cd $R; python3 tools/prof_summary.py /tmp/kt5 > $RES/r05_500k_kernel_trace_$1.txt; head -16 $RES/r05_500k_kernel_trace_$1.txt | cut -c1-190
