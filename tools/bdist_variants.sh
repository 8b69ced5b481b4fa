# k_bdist timing builds (results are garbage; GPU box): the default library,
# then MPCMMD_BDIST_VARIANT=1 (no mirror phase) and =2 (no stores at all),
# k_bdist ms per configs[1] step from bench.py's per-kernel times.
# The variants are tools/exp_bdist_variant.patch (csrc/k_bdist.hip): apply it
# in a scratch copy, build there, copy the libraries here, run this script:
#   cp -r mpc-mmd_amd include tools /tmp/bd && (cd /tmp/bd && git apply tools/exp_bdist_variant.patch)
#   make -C /tmp/bd/mpc-mmd_amd LIB=libmpcmmd_bd1.so BUILD=build_bd1 EXTRA=-DMPCMMD_BDIST_VARIANT=1 (and 2)
#   cp /tmp/bd/mpc-mmd_amd/libmpcmmd_bd?.so mpc-mmd_amd/
cd "${GRAFT_REPO_ROOT:-/root/repo}"
OUT=$(mktemp -d)
for lib in mpc-mmd_amd/libmpcmmd.so mpc-mmd_amd/libmpcmmd_bd1.so mpc-mmd_amd/libmpcmmd_bd2.so; do
  MPCMMD_LIB=$lib timeout -k 10 300 python bench.py --steps 6 --warmup 2 --full --extra 0 --cpu-seconds 0 > "$OUT/bd.json" 2> "$OUT/bd.err" || { tail -5 "$OUT/bd.err"; exit 1; }
  python3 -c "import json; d=json.load(open('$OUT/bd.json')); print('$lib', 'bdist ms/step', round(d['kernels_ms_per_step']['bdist'], 3))"
done
