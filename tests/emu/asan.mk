# TEST INFRASTRUCTURE ONLY: the emulator build under AddressSanitizer (CPU). GPU sanitizer builds are not allowed, so this is
# a host-only build with ROCm's clang: -fno-gpu-sanitize states that no device code is instrumented (there is none here).
#   make -C tests/emu -f asan.mk && tools/asan_emu.sh
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
SRC  := $(HERE)../../sh-assembly_amd/csrc
CLANGXX ?= $(or $(ROCM_PATH),/opt/rocm)/llvm/bin/clang++
$(HERE)libshk_emu_asan.so: $(SRC)/shk_api.hip $(SRC)/kmer_kernels.hip $(SRC)/partition_kernels.hip $(SRC)/cqf_kernels.hip $(SRC)/merge2_kernels.hip $(SRC)/walk_kernels.hip $(SRC)/unitig_kernels.hip $(SRC)/shk_device.h $(HERE)hip/hip_runtime.h $(HERE)emu_runtime.cpp $(HERE)../../include/shk.h
	$(CLANGXX) -std=c++20 -O1 -g -fsanitize=address -fno-gpu-sanitize -Wno-unused-command-line-argument -fno-omit-frame-pointer -fPIC -shared -Wno-unknown-pragmas -I$(HERE) -x c++ $(SRC)/shk_api.hip $(HERE)emu_runtime.cpp -o $@ -lpthread
