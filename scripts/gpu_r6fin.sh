# Round-6 close-out: GPU suite, smoke, the driver's bench command (config 2),
# the same under rocprofv3, every config's N = 1 line.  One step per limit.
set -o pipefail
O=${1:-r6fin}
bash scripts/gpu_r4.sh $O suite smoke && \
bash scripts/gpu_r4.sh $O bench:2:--gpus,1,--steps,20,--warmup,5 && \
bash scripts/gpu_r4.sh $O prof:2 bench:3 bench:4 bench:5 bench:5:--channel,rayleigh_mp
