# Builds libtrh.so (HIP kernels + C ABI, gfx950 only) and the oracle's C++ restatement.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
PKG := tiny-ram-halo2_amd
CSRC := $(PKG)/csrc
# build id = hash of the library's sources (trh_version() reports it)
BUILD_ID := $(shell cat $(CSRC)/*.hip $(CSRC)/*.h include/trh.h | sha1sum | cut -c1-12)
HIPFLAGS ?= -O3 -std=c++17 --offload-arch=$(ARCH) -fPIC -Wall -Wno-unused-function -Wno-unused-result
OBJS := $(CSRC)/capi.o $(CSRC)/msm.o $(CSRC)/ntt.o $(CSRC)/ipa.o $(CSRC)/ipafold.o $(CSRC)/ipaverify.o $(CSRC)/pointfft.o $(CSRC)/domain.o $(CSRC)/scan.o $(CSRC)/expr.o $(CSRC)/lookup.o $(CSRC)/hostio.o $(CSRC)/selftest.o $(CSRC)/encoding.o $(CSRC)/random.o $(CSRC)/permutation.o $(CSRC)/hashtocurve.o $(CSRC)/mockcheck.o $(CSRC)/quotient.o $(CSRC)/witness.o
HDRS := $(CSRC)/field.h $(CSRC)/fieldsqrt.h $(CSRC)/chacha.h $(CSRC)/blake2b.h $(CSRC)/transcript.h $(CSRC)/hashtocurve.h $(CSRC)/hashtocurve_consts.h $(CSRC)/curve.h $(CSRC)/curve_q4.h $(CSRC)/devmem.h $(CSRC)/dispatch.h $(CSRC)/ctx.h $(CSRC)/hostcombine.h $(CSRC)/hosthelper.h $(CSRC)/hostplan.h $(CSRC)/foldplan.h $(CSRC)/copypool.h $(CSRC)/devpool.h $(CSRC)/permkeygen.h $(CSRC)/tuplehash.h $(CSRC)/witness.h $(CSRC)/selftest_kat.h include/trh.h

all: $(PKG)/libtrh.so oracle examples/replay tests/native/multi_ctx_test tests/native/libtrh_q4broken.so tests/native/lazy29_dev_test tests/native/lazy29_alias_test tests/native/lazy29_segment_test tests/native/params_io_test tests/native/rng_fill_test tests/native/foldplan_test tests/native/perm_assembly_test tests/native/permkeygen_test tests/native/hashtocurve_vec_test tests/native/params_new_test tests/native/mock_check_test tests/native/quotient_test tests/native/transcript_test tests/native/witness_vec_test tests/native/witness_test

$(CSRC)/%.o: $(CSRC)/%.hip $(HDRS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# capi.o carries the build id: rebuilt whenever any source of the library changes
$(CSRC)/capi.o: $(CSRC)/capi.hip $(HDRS) $(wildcard $(CSRC)/*.hip)
	$(HIPCC) $(HIPFLAGS) -DTRH_BUILD_ID='"$(BUILD_ID)"' -c $< -o $@

$(PKG)/libtrh.so: $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $(OBJS) -ldl -o $@

# The library WITHOUT curve_q4.h's work-around for the ROCm 7.2 DPP-combiner miscompile: trh_init's self-test has to refuse it
# (tests/test_gpu_selftest.py).  Only the two objects that instantiate the quad-lane group law are rebuilt.
$(CSRC)/%.q4b.o: $(CSRC)/%.hip $(HDRS)
	$(HIPCC) $(HIPFLAGS) -DTRH_TEST_DROP_Q4_WORKAROUND -DTRH_BUILD_ID='"$(BUILD_ID)-q4broken"' -c $< -o $@
tests/native/libtrh_q4broken.so: $(CSRC)/capi.q4b.o $(CSRC)/msm.q4b.o $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $(CSRC)/capi.q4b.o $(CSRC)/msm.q4b.o $(filter-out $(CSRC)/capi.o $(CSRC)/msm.o,$(OBJS)) -ldl -o $@

# native (C++17, no Python) driver over include/trh.hpp
examples/replay: examples/replay.cpp include/trh.hpp include/trh.h $(PKG)/libtrh.so
	g++ -O2 -std=c++17 -Wall -Iinclude $< -o $@ -L$(PKG) -ltrh -pthread -Wl,-rpath,'$$ORIGIN/../$(PKG)'

# native test of the context layer (device group, per-thread contexts); run by tests/test_gpu_native.py
tests/native/multi_ctx_test: tests/native/multi_ctx_test.cpp include/trh.h $(PKG)/libtrh.so
	g++ -O1 -std=c++17 -Wall -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include $< -o $@ -L$(PKG) -ltrh -L/opt/rocm/lib -lamdhip64 -pthread \
	    -Wl,-rpath,'$$ORIGIN/../../$(PKG)' -Wl,-rpath,/opt/rocm/lib

# native round trip of Params::write / Params::read over include/trh.hpp; run by tests/test_gpu_encoding.py
tests/native/params_io_test: tests/native/params_io_test.cpp include/trh.hpp include/trh.h $(PKG)/libtrh.so
	g++ -O1 -std=c++17 -Wall -Iinclude $< -o $@ -L$(PKG) -ltrh -pthread -Wl,-rpath,'$$ORIGIN/../../$(PKG)'

# trh::Rng (the random-scalar stream) over include/trh.hpp; run by tests/test_gpu_rng.py
tests/native/rng_fill_test: tests/native/rng_fill_test.cpp include/trh.hpp include/trh.h $(PKG)/libtrh.so
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

# trh::PermutationAssembly (permutation keygen) over include/trh.hpp; run by tests/test_gpu_permkeygen.py
tests/native/perm_assembly_test: tests/native/perm_assembly_test.cpp include/trh.hpp include/trh.h $(PKG)/libtrh.so
	g++ -O1 -std=c++17 -Wall -Iinclude $< -o $@ -L$(PKG) -ltrh -pthread -Wl,-rpath,'$$ORIGIN/../../$(PKG)'

# the keygen assembly (csrc/permkeygen.h) on the host, under address + undefined sanitizers: reads copies, writes the mappings; run by
# tests/test_permkeygen_host.py (which checks them against the model and a union-find)
tests/native/permkeygen_test: tests/native/permkeygen_test.cpp $(CSRC)/permkeygen.h include/trh.h
	g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all $< -o $@

# csrc/blake2b.h and csrc/hashtocurve.h (hash_to_curve) on the host, under address + undefined sanitizers: reads inputs, writes digests,
# field elements and points; run by tests/test_hashtocurve_host.py (which checks them against hashlib and tests/hash_to_curve_model.py)
tests/native/hashtocurve_vec_test: tests/native/hashtocurve_vec_test.cpp $(CSRC)/blake2b.h $(CSRC)/hashtocurve.h $(CSRC)/hashtocurve_consts.h $(CSRC)/chacha.h $(CSRC)/fieldsqrt.h $(CSRC)/curve.h $(CSRC)/field.h
	g++ -O1 -g -std=c++17 -Wall -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=all $< -o $@

# trh::Params::create (Params::new: hash_to_curve on the device) over include/trh.hpp; run by tests/test_gpu_hashtocurve.py
tests/native/params_new_test: tests/native/params_new_test.cpp include/trh.hpp include/trh.h $(PKG)/libtrh.so
	g++ -O1 -std=c++17 -Wall -Iinclude $< -o $@ -L$(PKG) -ltrh -pthread -Wl,-rpath,'$$ORIGIN/../../$(PKG)'

# trh::GateEvaluator::check and trh::lookup_check (MockProver's gate and lookup checks) over include/trh.hpp; run by tests/test_gpu_mock.py
tests/native/mock_check_test: tests/native/mock_check_test.cpp include/trh.hpp include/trh.h $(PKG)/libtrh.so
	g++ -O1 -std=c++17 -Wall -Iinclude $< -o $@ -L$(PKG) -ltrh -pthread -Wl,-rpath,'$$ORIGIN/../../$(PKG)'

# trh::QuotientTerms (the permutation and lookup terms of h(X)) over include/trh.hpp; run by tests/test_gpu_quotient.py
tests/native/quotient_test: tests/native/quotient_test.cpp include/trh.hpp include/trh.h $(PKG)/libtrh.so
	g++ -O1 -std=c++17 -Wall -Iinclude $< -o $@ -L$(PKG) -ltrh -pthread -Wl,-rpath,'$$ORIGIN/../../$(PKG)'

# csrc/blake2b.h with a personalisation, csrc/transcript.h (the proof transcript) and trh::Blake2bWrite / Blake2bRead of include/trh.hpp on
# the host, under address + undefined sanitizers; the program defines the trh_tr_* entries itself (transcript_abi.cpp) and never loads libtrh;
# run by tests/test_transcript_host.py (which checks it against hashlib and tests/transcript_model.py)
tests/native/transcript_test: tests/native/transcript_test.cpp tests/native/transcript_abi.cpp include/trh.hpp include/trh.h $(CSRC)/transcript.h $(CSRC)/blake2b.h $(CSRC)/chacha.h $(CSRC)/fieldsqrt.h $(CSRC)/curve.h $(CSRC)/dispatch.h $(CSRC)/field.h
	g++ -O1 -g -std=c++17 -Wall -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=all tests/native/transcript_test.cpp tests/native/transcript_abi.cpp -o $@

# csrc/witness.h (integers to field elements, the even-bits decomposition) on the host, under address + undefined sanitizers: reads cases,
# prints limbs; never loads libtrh; run by tests/test_witness_host.py (which checks it against Python integers)
tests/native/witness_vec_test: tests/native/witness_vec_test.cpp $(CSRC)/witness.h $(CSRC)/field.h
	g++ -O1 -g -std=c++17 -Wall -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=all $< -o $@

# trh::columns_from_ints, trh::even_odd_split and trh::even_bits_table over include/trh.hpp; run by tests/test_gpu_witness.py
tests/native/witness_test: tests/native/witness_test.cpp include/trh.hpp include/trh.h $(PKG)/libtrh.so
	g++ -O1 -std=c++17 -Wall -Iinclude $< -o $@ -L$(PKG) -ltrh -pthread -Wl,-rpath,'$$ORIGIN/../../$(PKG)'

oracle:
	$(MAKE) -s -C oracle libtrh_oracle.so

clean:
	rm -f $(OBJS) $(CSRC)/*.q4b.o $(PKG)/libtrh.so tests/native/libtrh_q4broken.so examples/replay tests/native/multi_ctx_test tests/native/lazy29_dev_test tests/native/lazy29_alias_test tests/native/lazy29_segment_test tests/native/params_io_test tests/native/rng_fill_test tests/native/foldplan_test tests/native/perm_assembly_test tests/native/permkeygen_test tests/native/hashtocurve_vec_test tests/native/params_new_test tests/native/mock_check_test tests/native/quotient_test tests/native/transcript_test tests/native/witness_vec_test tests/native/witness_test
	$(MAKE) -s -C oracle clean

.PHONY: all oracle clean
