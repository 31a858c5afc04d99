# Builds libtrh.so (HIP kernels + C ABI, gfx950 only) and the oracle's C++ restatement.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
PKG := tiny-ram-halo2_amd
CSRC := $(PKG)/csrc
# build id = hash of the library's sources (trh_version() reports it)
BUILD_ID := $(shell cat $(CSRC)/*.hip $(CSRC)/*.h include/trh.h | sha1sum | cut -c1-12)
HIPFLAGS ?= -O3 -std=c++17 --offload-arch=$(ARCH) -fPIC -Wall -Wno-unused-function -Wno-unused-result
# every .hip under csrc/ is part of the library, every header there a prerequisite of every object
SRCS := $(wildcard $(CSRC)/*.hip)
OBJS := $(patsubst %.hip,%.o,$(SRCS))
HDRS := $(wildcard $(CSRC)/*.h) include/trh.h
ID_OBJ := $(CSRC)/capi.o
# driver programs over include/trh.hpp that share one command line, each run by the GPU test of its subject: Params::write / read
# (test_gpu_encoding.py), trh::Rng (test_gpu_rng.py), trh::PermutationAssembly (test_gpu_permkeygen.py), trh::Params::create
# (test_gpu_hashtocurve.py), GateEvaluator::check and lookup_check (test_gpu_mock.py), trh::QuotientTerms (test_gpu_quotient.py),
# columns_from_ints / even_odd_split / even_bits_table (test_gpu_witness.py), trh::mem_table (test_gpu_memtable.py),
# trh::exe_table (test_gpu_exetable.py), trh::exe_chips (test_gpu_exechips.py)
HPP_TESTS := $(addprefix tests/native/,params_io_test rng_fill_test perm_assembly_test params_new_test mock_check_test quotient_test witness_test memtable_test exetable_test \
    exechips_test)
NATIVE := examples/replay tests/native/libtrh_q4broken.so $(HPP_TESTS) $(addprefix tests/native/,multi_ctx_test lazy29_dev_test lazy29_alias_test lazy29_segment_test \
    foldplan_test permkeygen_test hashtocurve_vec_test transcript_test witness_vec_test memtable_vec_test exetable_vec_test exechips_vec_test)

all: $(PKG)/libtrh.so oracle $(NATIVE)

$(CSRC)/%.o: $(CSRC)/%.hip $(HDRS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# this object carries the build id: rebuilt whenever any source of the library changes
$(ID_OBJ): $(ID_OBJ:.o=.hip) $(HDRS) $(SRCS)
	$(HIPCC) $(HIPFLAGS) -DTRH_BUILD_ID='"$(BUILD_ID)"' -c $< -o $@

$(PKG)/libtrh.so: $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $(OBJS) -ldl -o $@

# The library WITHOUT curve_q4.h's work-around for the ROCm 7.2 DPP-combiner miscompile: trh_init's self-test has to refuse it
# (tests/test_gpu_selftest.py).  Only the objects that instantiate the quad-lane group law (they include curve_q4.h) and the one with the
# build id are rebuilt.
Q4B_OBJS := $(patsubst %.hip,%.o,$(shell grep -l 'include "curve_q4.h"' $(SRCS))) $(ID_OBJ)
$(CSRC)/%.q4b.o: $(CSRC)/%.hip $(HDRS)
	$(HIPCC) $(HIPFLAGS) -DTRH_TEST_DROP_Q4_WORKAROUND -DTRH_BUILD_ID='"$(BUILD_ID)-q4broken"' -c $< -o $@
tests/native/libtrh_q4broken.so: $(Q4B_OBJS:.o=.q4b.o) $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $(Q4B_OBJS:.o=.q4b.o) $(filter-out $(Q4B_OBJS),$(OBJS)) -ldl -o $@

# native (C++17, no Python) driver over include/trh.hpp
examples/replay: examples/replay.cpp include/trh.hpp include/trh.h $(PKG)/libtrh.so
	g++ -O2 -std=c++17 -Wall -Iinclude $< -o $@ -L$(PKG) -ltrh -pthread -Wl,-rpath,'$$ORIGIN/../$(PKG)'

# native test of the context layer (device group, per-thread contexts); run by tests/test_gpu_native.py
tests/native/multi_ctx_test: tests/native/multi_ctx_test.cpp include/trh.h $(PKG)/libtrh.so
	g++ -O1 -std=c++17 -Wall -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include $< -o $@ -L$(PKG) -ltrh -L/opt/rocm/lib -lamdhip64 -pthread \
	    -Wl,-rpath,'$$ORIGIN/../../$(PKG)' -Wl,-rpath,/opt/rocm/lib

$(HPP_TESTS): tests/native/%: tests/native/%.cpp include/trh.hpp include/trh.h $(PKG)/libtrh.so
	g++ -O1 -std=c++17 -Wall -Iinclude $< -o $@ -L$(PKG) -ltrh -pthread -Wl,-rpath,'$$ORIGIN/../../$(PKG)'

# the lazy 29-bit domain (field.h Fy, curve.h XYZZz) record by record on the device, compiled with the library's flags so that every
# operation is generated as in its kernels; run by tests/test_gpu_lazy29.py
tests/native/lazy29_dev_test: tests/native/lazy29_dev_test.hip tests/native/lazy29_cases.h $(CSRC)/field.h $(CSRC)/fieldsqrt.h $(CSRC)/curve.h
	$(HIPCC) $(HIPFLAGS) $< -o $@

# the product forms of the lazy domain with the result written over an operand and with shared operands; run by tests/test_gpu_lazy29_alias.py
tests/native/lazy29_alias_test: tests/native/lazy29_alias_test.hip tests/native/lazy29_cases.h $(CSRC)/field.h $(CSRC)/fieldsqrt.h $(CSRC)/curve.h
	$(HIPCC) $(HIPFLAGS) $< -o $@

# one segment of the accumulation (64 lanes x 128 mixed additions), every step against the host branch; run by tests/test_gpu_lazy29_segment.py
tests/native/lazy29_segment_test: tests/native/lazy29_segment_test.hip $(CSRC)/field.h $(CSRC)/fieldsqrt.h $(CSRC)/curve.h
	$(HIPCC) $(HIPFLAGS) $< -o $@

# the bucket lists of the generator collapse (csrc/foldplan.h) on the host, under address + undefined sanitizers: reads scalars, writes
# the plans; run by tests/test_foldplan.py (which checks them with big integers)
tests/native/foldplan_test: tests/native/foldplan_test.cpp $(CSRC)/foldplan.h $(CSRC)/hostcombine.h
	g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all $< -o $@

# the keygen assembly (csrc/permkeygen.h) on the host, under address + undefined sanitizers: reads copies, writes the mappings; run by
# tests/test_permkeygen_host.py (which checks them against the model and a union-find)
tests/native/permkeygen_test: tests/native/permkeygen_test.cpp $(CSRC)/permkeygen.h include/trh.h
	g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all $< -o $@

# csrc/blake2b.h and csrc/hashtocurve.h (hash_to_curve) on the host, under address + undefined sanitizers: reads inputs, writes digests,
# field elements and points; run by tests/test_hashtocurve_host.py (which checks them against hashlib and tests/hash_to_curve_model.py)
tests/native/hashtocurve_vec_test: tests/native/hashtocurve_vec_test.cpp $(CSRC)/blake2b.h $(CSRC)/hashtocurve.h $(CSRC)/hashtocurve_consts.h $(CSRC)/chacha.h $(CSRC)/fieldsqrt.h $(CSRC)/curve.h $(CSRC)/field.h
	g++ -O1 -g -std=c++17 -Wall -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=all $< -o $@

# csrc/blake2b.h with a personalisation, csrc/transcript.h (the proof transcript) and trh::Blake2bWrite / Blake2bRead of include/trh.hpp on
# the host, under address + undefined sanitizers; the program defines the trh_tr_* entries itself (transcript_abi.cpp) and never loads libtrh;
# run by tests/test_transcript_host.py (which checks it against hashlib and tests/transcript_model.py)
tests/native/transcript_test: tests/native/transcript_test.cpp tests/native/transcript_abi.cpp include/trh.hpp include/trh.h $(CSRC)/transcript.h $(CSRC)/blake2b.h $(CSRC)/chacha.h $(CSRC)/fieldsqrt.h $(CSRC)/curve.h $(CSRC)/dispatch.h $(CSRC)/field.h
	g++ -O1 -g -std=c++17 -Wall -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=all tests/native/transcript_test.cpp tests/native/transcript_abi.cpp -o $@

# csrc/witness.h (integers to field elements, the even-bits decomposition) on the host, under address + undefined sanitizers: reads cases,
# prints limbs; never loads libtrh; run by tests/test_witness_host.py (which checks it against Python integers)
tests/native/witness_vec_test: tests/native/witness_vec_test.cpp $(CSRC)/witness.h $(CSRC)/field.h
	g++ -O1 -g -std=c++17 -Wall -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=all $< -o $@

# csrc/memtable.h (the Mem table's plan, the rule of a log record, one row's thirteen integers) on the host, under address + undefined
# sanitizers: reads cases, prints results; never loads libtrh; run by tests/test_memtable_host.py (which checks it against
# tests/memtable_model.py)
tests/native/memtable_vec_test: tests/native/memtable_vec_test.cpp $(CSRC)/memtable.h $(CSRC)/witness.h $(CSRC)/field.h
	g++ -O1 -g -std=c++17 -Wall -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=all $< -o $@

# csrc/exetable.h (the Exe table's instruction decode, the rules of a selection table and of a step, one row's values and one-hot selectors)
# on the host, under address + undefined sanitizers: reads cases, prints results; never loads libtrh; run by tests/test_exetable_host.py
# (which checks it against tests/exetable_model.py)
tests/native/exetable_vec_test: tests/native/exetable_vec_test.cpp $(CSRC)/exetable.h $(CSRC)/witness.h $(CSRC)/field.h include/trh.h
	g++ -O1 -g -std=c++17 -Wall -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=all $< -o $@

# the chips part of csrc/exetable.h (the layout, the rules of a chips table, one row's cells) on the host, under address + undefined
# sanitizers: reads cases, prints results; never loads libtrh; run by tests/test_exechips_host.py (which checks it against
# tests/exechips_model.py)
tests/native/exechips_vec_test: tests/native/exechips_vec_test.cpp $(CSRC)/exetable.h $(CSRC)/witness.h $(CSRC)/field.h include/trh.h
	g++ -O1 -g -std=c++17 -Wall -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=all $< -o $@

# the inversion kernel of trh_exe_chips_dev (csrc/exechips_inv.h) at strips of 1, 4 and 8 rows per lane, timed on its own; not part of
# `all`: tools/exechips_probe.py runs it when it has been built
tools/exechips_inv_probe: tools/exechips_inv_probe.hip $(HDRS)
	$(HIPCC) $(HIPFLAGS) $< -o $@

oracle:
	$(MAKE) -s -C oracle libtrh_oracle.so

clean:
	rm -f $(OBJS) $(CSRC)/*.q4b.o $(PKG)/libtrh.so $(NATIVE)
	$(MAKE) -s -C oracle clean

.PHONY: all oracle clean
