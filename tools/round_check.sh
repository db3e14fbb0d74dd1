#!/bin/bash
# Full GPU check of the current tree: GPU tests, a default --full bench line,
# then the profile passes (kernel trace + Hessian FETCH/WRITE) under a tag.
# Logs go to $CHECK_OUT (default check_out/).
#   bash tools/round_check.sh <tag>
set -u
TAG=${1:-rXX}
cd /tmp && export TMPDIR=/tmp
cd "${GRAFT_REPO_ROOT:-/root/repo}"
O=${CHECK_OUT:-check_out}
mkdir -p $O
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $O/rc_${TAG}_pytest.log 2>&1 || { tail -40 $O/rc_${TAG}_pytest.log; exit 1; }
tail -2 $O/rc_${TAG}_pytest.log
timeout -k 10 300 python -u bench.py --full > $O/rc_${TAG}_bench.json 2> $O/rc_${TAG}_bench.err || { tail -20 $O/rc_${TAG}_bench.err; exit 1; }
cat $O/rc_${TAG}_bench.json
bash tools/profile_round.sh ${TAG}
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke(); print('SMOKE_OK')" > $O/rc_${TAG}_smoke.log 2>&1 || { tail -20 $O/rc_${TAG}_smoke.log; exit 1; }
tail -1 $O/rc_${TAG}_smoke.log
