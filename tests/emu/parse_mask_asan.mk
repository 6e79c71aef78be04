# TEST INFRASTRUCTURE ONLY: parse_mask_asan.cpp and the kernel sources compiled for the CPU (see hip/hip_runtime.h) into one
# program under AddressSanitizer. GPU sanitizer builds are not allowed, so this is a host-only build with ROCm's clang, as
# asan.mk: -fno-gpu-sanitize states that no device code is instrumented (there is none here). Run on the CPU only.
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
SRC  := $(HERE)../../sh-assembly_amd/csrc
CLANGXX ?= $(or $(ROCM_PATH),/opt/rocm)/llvm/bin/clang++
$(HERE)parse_mask_asan: $(HERE)parse_mask_asan.cpp $(SRC)/shk_api.hip $(SRC)/kmer_kernels.hip $(SRC)/roll_kernels.hip $(SRC)/partition_kernels.hip $(SRC)/cqf_kernels.hip $(SRC)/merge2_kernels.hip $(SRC)/walk_kernels.hip $(SRC)/unitig_kernels.hip $(SRC)/shk_device.h $(HERE)hip/hip_runtime.h $(HERE)emu_runtime.cpp $(HERE)../../include/shk.h
	$(CLANGXX) -std=c++20 -O1 -g -fsanitize=address -fno-gpu-sanitize -Wno-unused-command-line-argument -fno-omit-frame-pointer -Wno-unknown-pragmas -I$(HERE) -x c++ $(HERE)parse_mask_asan.cpp $(SRC)/shk_api.hip $(HERE)emu_runtime.cpp -o $@ -lpthread
