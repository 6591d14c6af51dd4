# dev (round 6, one GPU call): parity of the one-launch RPN head, slide-level bench with documents, attention presplit probe
O=gpurun_out/r06c; mkdir -p $O
timeout 900 python -m pytest tests/test_hip_full.py tests/test_hip_edges.py -m gpu -x -q 2>&1 | grep -v amdgpu.ids | tail -5 > $O/parity.log; tail -2 $O/parity.log
timeout 600 python tools/bench_wsi.py > $O/bench_wsi.json 2> $O/bench_wsi.err; tail -c 900 $O/bench_wsi.json; echo
bash tools/dev/r06_attn_presplit.sh > $O/attn_presplit.log 2>&1; cp gpurun_out/r06_attn_presplit.txt $O/; tail -9 $O/r06_attn_presplit.txt
