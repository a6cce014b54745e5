# usage: OUT=<output directory, default out> bash tools/gpu_pmc.sh <tag> [batch] -- bench + kernel trace + PMC passes (separate runs,
# kernel-trace only)
TAG=${1:-pmc}; B=${2:-64}
OUT=${OUT:-out}
mkdir -p $OUT
export TMPDIR=/tmp
timeout 600 python bench.py --steps 10 --warmup 3 --batch $B --full --no-cpu-baseline > $OUT/${TAG}_bench_b$B.log 2>&1; echo "rc=$?" >> $OUT/${TAG}_bench_b$B.log
timeout 600 rocprofv3 --kernel-trace --stats -d $OUT/${TAG}_trace -o t -- python bench.py --steps 3 --warmup 2 --batch $B --no-cpu-baseline --no-profile > $OUT/${TAG}_trace.log 2>&1
python tools/rocpd_summary.py $OUT/${TAG}_trace/t_results.db --by-grid > $OUT/${TAG}_kernel_stats_by_grid.txt 2>&1
python tools/rocpd_summary.py $OUT/${TAG}_trace/t_results.db > $OUT/${TAG}_kernel_stats.txt 2>&1
rm -rf $OUT/${TAG}_trace
rocprofv3 -L > $OUT/${TAG}_counters_list.txt 2>&1
timeout 900 rocprofv3 --kernel-trace --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_VALU_MFMA_BUSY_CYCLES SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE -d $OUT/${TAG}_pmc1 -o p -- python bench.py --steps 1 --warmup 1 --batch $B --no-cpu-baseline --no-profile > $OUT/${TAG}_pmc1.log 2>&1; echo "rc=$?" >> $OUT/${TAG}_pmc1.log
timeout 900 rocprofv3 --kernel-trace --pmc FETCH_SIZE GRBM_GUI_ACTIVE -d $OUT/${TAG}_pmc2 -o p -- python bench.py --steps 1 --warmup 1 --batch $B --no-cpu-baseline --no-profile > $OUT/${TAG}_pmc2.log 2>&1; echo "rc=$?" >> $OUT/${TAG}_pmc2.log
timeout 900 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $OUT/${TAG}_pmc3 -o p -- python bench.py --steps 1 --warmup 1 --batch $B --no-cpu-baseline --no-profile > $OUT/${TAG}_pmc3.log 2>&1; echo "rc=$?" >> $OUT/${TAG}_pmc3.log
python tools/rocpd_pmc.py $OUT/${TAG}_pmc1/p_results.db > $OUT/${TAG}_pmc1.txt 2>&1
python tools/rocpd_pmc.py $OUT/${TAG}_pmc2/p_results.db > $OUT/${TAG}_pmc2.txt 2>&1
python tools/rocpd_pmc.py $OUT/${TAG}_pmc3/p_results.db > $OUT/${TAG}_pmc3.txt 2>&1
ls -la $OUT/${TAG}_pmc1 $OUT/${TAG}_pmc2
rm -rf $OUT/${TAG}_pmc2 $OUT/${TAG}_pmc3
grep -h '^{' $OUT/${TAG}_bench_b$B.log | cut -c1-1600
head -16 $OUT/${TAG}_kernel_stats.txt | cut -c1-190
head -30 $OUT/${TAG}_pmc1.txt | cut -c1-220
