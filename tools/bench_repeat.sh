# Five default 20-step bench runs back to back (run-to-run spread of the headline).
line=$(mktemp)
for rep in 1 2 3 4 5; do
  timeout -k 10 120 python3 bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-pipelined > "$line" 2>/dev/null || exit 1
  tail -1 "$line" | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print('rep $rep value %.4g ms %.4f'%(d['value'],d['ms_per_step']), 'step_ms', d['step_ms'], 'kernel_ms %.4f'%d['kernel_ms'])"
done
