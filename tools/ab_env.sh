# Dev helper (GPU box): ICP ms/iteration (configs[1] / configs[2]) under environment variants; AB_VARIANTS="VAR=a VAR=b ..."
# A variant may be another build of the library: LSN_NATIVE_LIB=path/to/libNativeUtils.so (made absolute here: the drivers change directory);
# the word `tree` stands for this tree's own library with nothing set.  AB_ROUNDS=n walks the list n times, so the variants alternate.
for round in $(seq ${AB_ROUNDS:-1}); do
for v in ${AB_VARIANTS}; do
  case $v in
    tree) set_v=_AB_NONE=1 ;;
    LSN_NATIVE_LIB=*) set_v=LSN_NATIVE_LIB=$(realpath "${v#LSN_NATIVE_LIB=}") ;;
    *) set_v=$v ;;
  esac
  for sens in 2 8; do
    echo "$v sensors=$sens: $(env $set_v ICP_SENSORS=$sens ICP_REPS=5 timeout -k 10 120 python tools/icp_driver.py 2>&1 | grep -E 'ms/iter' | awk '{printf "%s ", substr($6,1,7)}')"
  done
done
done
