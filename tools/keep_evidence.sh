#!/bin/bash
# usage: tools/keep_evidence.sh <tag> -- copy the evidence of tools/profile_round.sh from
# $PB_EVIDENCE_DIR (scratch, default evidence/) into profiles/ (tracked): bench lines, kernel stats,
# counters, logs; pmc_traffic.json is the file bench.py reads (accepted only when its hash is the
# library's).
tag=${1:-r04}
cd "$(dirname "$0")/.."
src=${PB_EVIDENCE_DIR:-evidence}
for f in $src/${tag}_*.json $src/${tag}_*.csv $src/${tag}_*.log $src/${tag}_library_*.txt; do
  [ -f "$f" ] && cp "$f" profiles/
done
[ -f $src/pmc_traffic.json ] && cp $src/pmc_traffic.json profiles/pmc_traffic.json
ls profiles | grep "^${tag}_" | wc -l
