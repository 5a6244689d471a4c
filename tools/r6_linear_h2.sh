cd $GRAFT_REPO_ROOT
for h in 1 0 1 0; do echo "== LINEAR_FWD_H2=$h"; YT8M_LINEAR_FWD_H2=$h python bench.py --full --workload netvlad --steps 30 --warmup 6 --no-cpu-baseline --no-gap --no-extra 2>/dev/null | python -c "
import sys,json
d=json.loads(sys.stdin.read()); print('%.4f ms/step' % d['ms_per_step'], {k:round(v['ms_per_step'],3) for k,v in d['roofline']['families'].items()})"; done
