# Builds the MI355X (gfx950) library and the CPU oracle.  `python -c "import __graft_entry__ as g; g.build()"`
# runs the same commands.  One object per source of ccfindr_amd/csrc (build/, git-ignored): every *.cpp as plain C++, every
# *.hip for gfx950 -- one unit per feature and per kernel family of the engine (engine, batch, mlnmf, svd, labels, hooks), each
# kernel in one unit, so a change to one of them recompiles that unit and not the others' kernels.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
CSRC := ccfindr_amd/csrc
LIB := ccfindr_amd/lib/libvbnmf_hip.so
OBJ := build/obj
CXXFLAGS ?= -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function -pthread
HIPFLAGS ?= $(CXXFLAGS) --offload-arch=$(ARCH)
DEV_HDRS := $(wildcard $(CSRC)/*.h) include/vbnmf.h
SOURCES := $(sort $(wildcard $(CSRC)/*.cpp) $(wildcard $(CSRC)/*.hip))
OBJECTS := $(patsubst $(CSRC)/%,$(OBJ)/%.o,$(basename $(SOURCES)))

all: $(LIB) oracle testlibs

$(OBJ)/%.o: $(CSRC)/%.cpp
	mkdir -p $(OBJ)
	$(HIPCC) $(CXXFLAGS) -MMD -c -o $@ $<

$(OBJ)/%.o: $(CSRC)/%.hip
	mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -MMD -c -o $@ -x hip $<

# An object's headers: the compiler's own list from its last compile (-MMD), so a header rebuilds the units that include it
# and no other; an object that has no such list yet depends on every header.
$(foreach o,$(OBJECTS),$(if $(wildcard $(o:.o=.d)),,$(eval $(o): $(DEV_HDRS))))
-include $(OBJECTS:.o=.d)

$(LIB): $(OBJECTS)
	mkdir -p $(dir $(LIB))
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -o $@ $^ -pthread

oracle:
	$(MAKE) -C oracle

# test infrastructure: the stand-in for librccl that lets two processes on ONE GPU run the library's RCCL protocol
testlibs:
	$(MAKE) -C tests/fake_rccl

clean:
	rm -rf ccfindr_amd/lib oracle/_build build tests/fake_rccl/_build
.PHONY: all oracle testlibs clean
