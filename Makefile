# Builds libpmc.so (HIP kernels + C ABI) for gfx950, in-tree.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
CSRC := parelagmc_amd/csrc
OBJDIR := build/obj
SRCS := $(CSRC)/k_sell.hip $(CSRC)/k_darcy.hip $(CSRC)/k_krylov.hip $(CSRC)/k_tail.hip $(CSRC)/k_fields.hip $(CSRC)/sparse.hip $(CSRC)/solver.hip $(CSRC)/sampler.hip $(CSRC)/darcy.hip $(CSRC)/darcy_gradient.hip $(CSRC)/darcy_hessian.hip $(CSRC)/newton_cg.hip $(CSRC)/capi.hip $(CSRC)/hybrid_build.hip $(CSRC)/kl.hip $(CSRC)/kl_adjoint.hip $(CSRC)/sampler_adjoint.hip $(CSRC)/kl_eigs.hip $(CSRC)/field_stats.hip $(CSRC)/level_fields.hip $(CSRC)/condition.hip $(CSRC)/tracer.hip $(CSRC)/transport.hip
OBJS := $(patsubst $(CSRC)/%.hip,$(OBJDIR)/%.o,$(SRCS))
HDRS := $(wildcard $(CSRC)/*.hpp) include/pmc.h
EXTRA ?=
CXXFLAGS := -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -Wall -Wno-unused-function $(EXTRA)
LIB := parelagmc_amd/lib/libpmc.so

all: $(LIB)

$(OBJDIR)/%.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(CXXFLAGS) -c $< -o $@

$(LIB): $(OBJS)
	@mkdir -p parelagmc_amd/lib
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -o $@ $(OBJS) -ldl

clean:
	rm -rf build parelagmc_amd/lib/libpmc.so

.PHONY: all clean

# host-side managers (plain C++, links against libpmc.so next to it)
HOSTLIB := parelagmc_amd/lib/libpmc_host.so
HOSTSRC := parelagmc_amd/host/host.cpp parelagmc_amd/host/mortar.cpp
$(HOSTLIB): $(HOSTSRC) parelagmc_amd/host/parelagmc.hpp include/pmc.h include/pmc_host.h $(LIB)
	g++ -O2 -std=c++17 -fPIC -shared -Wall -pthread -Iinclude -o $@ $(HOSTSRC) -Lparelagmc_amd/lib -lpmc -Wl,-rpath,'$$ORIGIN'

all: $(HOSTLIB)

# kernel laboratory (tuning only): links the library's objects with a main(); kept next to the library so that it travels
# to the GPU box (build/ does not)
LABBIN := parelagmc_amd/lib/k5_lab
$(OBJDIR)/k5_lab.o: scripts/lab/k5_lab.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(CXXFLAGS) -c $< -o $@
$(LABBIN): $(OBJDIR)/k5_lab.o $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -o $@ $(OBJDIR)/k5_lab.o $(OBJS) -ldl
lab: $(LABBIN)
.PHONY: lab

# laboratory build of the library: the same sources with -DPMC_LAB, i.e. with the PMC_* tuning overrides of csrc/common.hpp
# (lab_env) compiled in.  The product library (libpmc.so) reads none of them.  scripts/lab/*.sh copy it over libpmc.so on the
# GPU box's scratch tree for same-box A/B runs.
lab-lib:
	$(MAKE) OBJDIR=build/obj_lab LIB=parelagmc_amd/lib/libpmc_lab.so EXTRA="-DPMC_LAB $(LABEXTRA)" parelagmc_amd/lib/libpmc_lab.so
.PHONY: lab-lib

# Boundary tests compiled from C and C++ (tests/test_abi_binaries.py runs them): the C program sees include/pmc.h only,
# the C++ one the MFEM adapter (against tests/c/mfem_shim.hpp) and the mirror classes of parelagmc.hpp
ABIBIN := tests/c/bin
# (the libraries are order-only prerequisites: on a box that received the built .so files but not build/obj, nothing is rebuilt)
$(ABIBIN)/abi_smoke: tests/c/abi_smoke.c tests/c/prob_io.h include/pmc.h | $(LIB)
	@mkdir -p $(ABIBIN)
	gcc -std=c11 -O1 -Wall -Wextra -Werror -Iinclude -Itests/c -o $@ tests/c/abi_smoke.c -Lparelagmc_amd/lib -lpmc -lm -Wl,-rpath,'$$ORIGIN/../../../parelagmc_amd/lib'
$(ABIBIN)/adapter_smoke: tests/c/adapter_smoke.cpp tests/c/prob_io.h tests/c/mfem_shim.hpp parelagmc_amd/host/mfem_adapter.hpp parelagmc_amd/host/parelagmc.hpp include/pmc.h include/pmc_host.h | $(HOSTLIB)
	@mkdir -p $(ABIBIN)
	g++ -std=c++17 -O1 -Wall -Wextra -Iinclude -Itests/c -o $@ tests/c/adapter_smoke.cpp -Lparelagmc_amd/lib -lpmc_host -lpmc -pthread -Wl,-rpath,'$$ORIGIN/../../../parelagmc_amd/lib'
test-abi: $(ABIBIN)/abi_smoke $(ABIBIN)/adapter_smoke
.PHONY: test-abi

# KL sampler callers from C and C++ (tests/test_gpu_kl.py builds and runs them; test-abi above is unchanged)
$(ABIBIN)/kl_smoke: tests/c/kl_smoke.c tests/c/kl_io.h include/pmc.h | $(LIB)
	@mkdir -p $(ABIBIN)
	gcc -std=c11 -O1 -Wall -Wextra -Werror -Iinclude -Itests/c -o $@ tests/c/kl_smoke.c -Lparelagmc_amd/lib -lpmc -lm -Wl,-rpath,'$$ORIGIN/../../../parelagmc_amd/lib'
$(ABIBIN)/kl_adapter_smoke: tests/c/kl_adapter_smoke.cpp tests/c/kl_io.h tests/c/mfem_shim.hpp parelagmc_amd/host/mfem_adapter.hpp parelagmc_amd/host/parelagmc.hpp include/pmc.h include/pmc_host.h | $(HOSTLIB)
	@mkdir -p $(ABIBIN)
	g++ -std=c++17 -O1 -Wall -Wextra -Iinclude -Itests/c -o $@ tests/c/kl_adapter_smoke.cpp -Lparelagmc_amd/lib -lpmc_host -lpmc -pthread -Wl,-rpath,'$$ORIGIN/../../../parelagmc_amd/lib'
test-kl: $(ABIBIN)/kl_smoke $(ABIBIN)/kl_adapter_smoke
.PHONY: test-kl

# the drivers' result table from C and C++ (tests/test_gpu_field_stats.py builds and runs them)
$(ABIBIN)/field_stats_smoke: tests/c/field_stats_smoke.c tests/c/kl_io.h include/pmc.h | $(LIB)
	@mkdir -p $(ABIBIN)
	gcc -std=c11 -O1 -Wall -Wextra -Werror -Iinclude -Itests/c -o $@ tests/c/field_stats_smoke.c -Lparelagmc_amd/lib -lpmc -lm -Wl,-rpath,'$$ORIGIN/../../../parelagmc_amd/lib'
$(ABIBIN)/field_stats_adapter_smoke: tests/c/field_stats_adapter_smoke.cpp tests/c/kl_io.h tests/c/mfem_shim.hpp parelagmc_amd/host/mfem_adapter.hpp parelagmc_amd/host/parelagmc.hpp include/pmc.h include/pmc_host.h | $(HOSTLIB)
	@mkdir -p $(ABIBIN)
	g++ -std=c++17 -O1 -Wall -Wextra -Iinclude -Itests/c -o $@ tests/c/field_stats_adapter_smoke.cpp -Lparelagmc_amd/lib -lpmc_host -lpmc -pthread -Wl,-rpath,'$$ORIGIN/../../../parelagmc_amd/lib'
test-field-stats: $(ABIBIN)/field_stats_smoke $(ABIBIN)/field_stats_adapter_smoke
.PHONY: test-field-stats

# the multilevel pressure estimates from C (tests/test_gpu_pressure_stats.py builds and runs it)
$(ABIBIN)/pressure_stats_smoke: tests/c/pressure_stats_smoke.c tests/c/prob_io.h include/pmc.h include/pmc_host.h | $(HOSTLIB)
	@mkdir -p $(ABIBIN)
	gcc -std=c11 -O1 -Wall -Wextra -Werror -Iinclude -Itests/c -o $@ tests/c/pressure_stats_smoke.c -Lparelagmc_amd/lib -lpmc_host -lpmc -lm -Wl,-rpath,'$$ORIGIN/../../../parelagmc_amd/lib'
test-pressure-stats: $(ABIBIN)/pressure_stats_smoke
.PHONY: test-pressure-stats

# the posterior field estimates of the ratio managers from C (tests/test_gpu_posterior_fields.py builds and runs it)
$(ABIBIN)/posterior_fields_smoke: tests/c/posterior_fields_smoke.c tests/c/prob_io.h include/pmc.h include/pmc_host.h | $(HOSTLIB)
	@mkdir -p $(ABIBIN)
	gcc -std=c11 -O1 -Wall -Wextra -Werror -Iinclude -Itests/c -o $@ tests/c/posterior_fields_smoke.c -Lparelagmc_amd/lib -lpmc_host -lpmc -lm -Wl,-rpath,'$$ORIGIN/../../../parelagmc_amd/lib'
test-posterior-fields: $(ABIBIN)/posterior_fields_smoke
.PHONY: test-posterior-fields

# the device Matern eigensolver from C (tests/test_gpu_kl_eigs_c.py builds and runs it)
$(ABIBIN)/kl_matern_smoke: tests/c/kl_matern_smoke.c include/pmc.h | $(LIB)
	@mkdir -p $(ABIBIN)
	gcc -std=c11 -O1 -Wall -Wextra -Werror -Iinclude -Itests/c -o $@ tests/c/kl_matern_smoke.c -Lparelagmc_amd/lib -lpmc -lm -Wl,-rpath,'$$ORIGIN/../../../parelagmc_amd/lib'
test-kl-matern: $(ABIBIN)/kl_matern_smoke
.PHONY: test-kl-matern

# conditioning on observed field values from C (tests/test_gpu_condition.py builds and runs it)
$(ABIBIN)/condition_smoke: tests/c/condition_smoke.c tests/c/kl_io.h include/pmc.h | $(LIB)
	@mkdir -p $(ABIBIN)
	gcc -std=c11 -O1 -Wall -Wextra -Werror -Iinclude -Itests/c -o $@ tests/c/condition_smoke.c -Lparelagmc_amd/lib -lpmc -lm -Wl,-rpath,'$$ORIGIN/../../../parelagmc_amd/lib'
test-condition: $(ABIBIN)/condition_smoke
.PHONY: test-condition

# the tangent and adjoint of the conditioning map from C (tests/test_gpu_condition_derivatives.py builds and runs it)
$(ABIBIN)/condition_derivatives_smoke: tests/c/condition_derivatives_smoke.c tests/c/kl_io.h include/pmc.h | $(LIB)
	@mkdir -p $(ABIBIN)
	gcc -std=c11 -O1 -Wall -Wextra -Werror -Iinclude -Itests/c -o $@ tests/c/condition_derivatives_smoke.c -Lparelagmc_amd/lib -lpmc -lm -Wl,-rpath,'$$ORIGIN/../../../parelagmc_amd/lib'
test-condition-derivatives: $(ABIBIN)/condition_derivatives_smoke
.PHONY: test-condition-derivatives

# the adjoint gradients through the mirror classes of parelagmc.hpp (tests/test_gpu_darcy_gradient.py builds and runs it)
$(ABIBIN)/gradient_smoke: tests/c/gradient_smoke.cpp tests/c/prob_io.h parelagmc_amd/host/parelagmc.hpp include/pmc.h include/pmc_host.h | $(HOSTLIB)
	@mkdir -p $(ABIBIN)
	g++ -std=c++17 -O1 -Wall -Wextra -Iinclude -Itests/c -o $@ tests/c/gradient_smoke.cpp -Lparelagmc_amd/lib -lpmc_host -lpmc -pthread -Wl,-rpath,'$$ORIGIN/../../../parelagmc_amd/lib'
test-gradient: $(ABIBIN)/gradient_smoke
.PHONY: test-gradient

# the V-cycle's path decision (csrc/vcycle_plan.hpp) against the predicates it replaced: plain C++, no library, no device
# (tests/test_vcycle_plan.py builds and runs it)
$(ABIBIN)/vcycle_plan_check: tests/c/vcycle_plan_check.cpp $(CSRC)/vcycle_plan.hpp
	@mkdir -p $(ABIBIN)
	g++ -std=c++17 -O2 -Wall -Wextra -Werror -I$(CSRC) -o $@ tests/c/vcycle_plan_check.cpp
test-vcycle-plan: $(ABIBIN)/vcycle_plan_check
.PHONY: test-vcycle-plan

# the adjoint of Eval from C (tests/test_gpu_sampler_adjoint.py builds and runs it)
$(ABIBIN)/sampler_adjoint_smoke: tests/c/sampler_adjoint_smoke.c tests/c/prob_io.h include/pmc.h | $(LIB)
	@mkdir -p $(ABIBIN)
	gcc -std=c11 -O1 -Wall -Wextra -Werror -Iinclude -Itests/c -o $@ tests/c/sampler_adjoint_smoke.c -Lparelagmc_amd/lib -lpmc -lm -Wl,-rpath,'$$ORIGIN/../../../parelagmc_amd/lib'
test-sampler-adjoint: $(ABIBIN)/sampler_adjoint_smoke
.PHONY: test-sampler-adjoint

# the Gauss-Newton Hessian action through the mirror classes of parelagmc.hpp (tests/test_gpu_darcy_gn_hessian.py builds and
# runs it)
$(ABIBIN)/gn_hessian_smoke: tests/c/gn_hessian_smoke.cpp tests/c/prob_io.h parelagmc_amd/host/parelagmc.hpp include/pmc.h include/pmc_host.h | $(HOSTLIB)
	@mkdir -p $(ABIBIN)
	g++ -std=c++17 -O1 -Wall -Wextra -Iinclude -Itests/c -o $@ tests/c/gn_hessian_smoke.cpp -Lparelagmc_amd/lib -lpmc_host -lpmc -pthread -Wl,-rpath,'$$ORIGIN/../../../parelagmc_amd/lib'
test-gn-hessian: $(ABIBIN)/gn_hessian_smoke
.PHONY: test-gn-hessian

# MAP estimation through the mirror classes of parelagmc.hpp (tests/test_gpu_map_estimate.py builds and runs it)
$(ABIBIN)/map_smoke: tests/c/map_smoke.cpp tests/c/prob_io.h parelagmc_amd/host/parelagmc.hpp include/pmc.h include/pmc_host.h | $(HOSTLIB)
	@mkdir -p $(ABIBIN)
	g++ -std=c++17 -O1 -Wall -Wextra -Iinclude -Itests/c -o $@ tests/c/map_smoke.cpp -Lparelagmc_amd/lib -lpmc_host -lpmc -pthread -Wl,-rpath,'$$ORIGIN/../../../parelagmc_amd/lib'
test-map: $(ABIBIN)/map_smoke
.PHONY: test-map
