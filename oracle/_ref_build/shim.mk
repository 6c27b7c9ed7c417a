# TESTS ONLY: the header-only shim include/BatchScenarioExp.h compiled inside the REFERENCE'S header tree (unchanged scenarios/Scenario.h,
# learning/ExpTuple.h, util/ArgParser.h from $(REF); stand-in Eigen from oracle/_ref_build/stubs), linked once against the lane-loop test
# backend (CPU tests) and once against the HIP library (the -m gpu test runs that prebuilt binary where $(REF) is absent).
# Sources: tests/shim/*.cpp. Outputs: oracle/_ref/shim/ (git-ignored, next to the other reference builds). Run through the Makefile beside it
# (make -C oracle/_ref_build shim), which passes REF.
CXX ?= g++
REPO := ../..
SRC := $(REPO)/tests/shim
OUT := $(REPO)/oracle/_ref/shim
REF_SRC := $(REF)/scenarios/Scenario.cpp $(REF)/learning/ExpTuple.cpp $(REF)/util/ArgParser.cpp $(REF)/util/FileUtil.cpp $(REF)/util/MathUtil.cpp $(REF)/util/Rand.cpp
CXXFLAGS := -std=c++17 -O1 -D_LINUX_ -DNDEBUG -w -I$(REPO)/include -I$(REPO)/oracle/_ref_build/stubs -I$(REF)
EMUL_RPATH := -Wl,-rpath,'$$ORIGIN/../../../tests/emul'
HIP_RPATH := -Wl,-rpath,'$$ORIGIN/../../../deepterrainrl_amd/lib' -Wl,-rpath,/opt/rocm/lib

all:
	@if [ -n "$(REF)" ] && [ -d "$(REF)/scenarios" ]; then mkdir -p $(OUT) && $(MAKE) --no-print-directory -f shim.mk $(addprefix $(OUT)/,drive_shim_emul drive_shim_hip drive_shim_eval_emul drive_shim_eval_hip drive_shim_net_emul drive_shim_net_hip); else echo "shim drivers: $(REF) not present, keeping the prebuilt drivers"; fi

$(OUT)/drive_shim_emul: $(SRC)/drive_shim.cpp $(REPO)/include/BatchScenarioExp.h $(REPO)/include/dtrl.h $(REPO)/tests/emul/libdtrl_emul.so
	$(CXX) $(CXXFLAGS) -o $@ $(SRC)/drive_shim.cpp $(REF_SRC) -L$(REPO)/tests/emul -ldtrl_emul $(EMUL_RPATH) -lpthread

$(OUT)/drive_shim_hip: $(SRC)/drive_shim.cpp $(REPO)/include/BatchScenarioExp.h $(REPO)/include/dtrl.h $(REPO)/deepterrainrl_amd/lib/libdtrl.so
	$(CXX) $(CXXFLAGS) -o $@ $(SRC)/drive_shim.cpp $(REF_SRC) -L$(REPO)/deepterrainrl_amd/lib -ldtrl $(HIP_RPATH) -L/opt/rocm/lib -lamdhip64

# include/BatchScenarioPoliEval.h : cScenario, the same two ways
$(OUT)/drive_shim_eval_emul: $(SRC)/drive_shim_eval.cpp $(REPO)/include/BatchScenarioPoliEval.h $(REPO)/include/dtrl.h $(REPO)/tests/emul/libdtrl_emul.so
	$(CXX) $(CXXFLAGS) -o $@ $(SRC)/drive_shim_eval.cpp $(REF_SRC) -L$(REPO)/tests/emul -ldtrl_emul $(EMUL_RPATH) -lpthread

$(OUT)/drive_shim_eval_hip: $(SRC)/drive_shim_eval.cpp $(REPO)/include/BatchScenarioPoliEval.h $(REPO)/include/dtrl.h $(REPO)/deepterrainrl_amd/lib/libdtrl.so
	$(CXX) $(CXXFLAGS) -o $@ $(SRC)/drive_shim_eval.cpp $(REF_SRC) -L$(REPO)/deepterrainrl_amd/lib -ldtrl $(HIP_RPATH) -L/opt/rocm/lib -lamdhip64

# include/BatchNeuralNet.h (cNeuralNet's interface over the native trainer step), the same two ways
$(OUT)/drive_shim_net_emul: $(SRC)/drive_shim_net.cpp $(REPO)/include/BatchNeuralNet.h $(REPO)/include/dtrl_trainer.h $(REPO)/tests/emul/libdtrl_trainer_emul.so
	$(CXX) $(CXXFLAGS) -o $@ $(SRC)/drive_shim_net.cpp $(REF)/util/MathUtil.cpp $(REF)/util/Rand.cpp -L$(REPO)/tests/emul -ldtrl_trainer_emul $(EMUL_RPATH) -lpthread

$(OUT)/drive_shim_net_hip: $(SRC)/drive_shim_net.cpp $(REPO)/include/BatchNeuralNet.h $(REPO)/include/dtrl_trainer.h $(REPO)/deepterrainrl_amd/lib/libdtrl.so
	$(CXX) $(CXXFLAGS) -o $@ $(SRC)/drive_shim_net.cpp $(REF)/util/MathUtil.cpp $(REF)/util/Rand.cpp -L$(REPO)/deepterrainrl_amd/lib -ldtrl $(HIP_RPATH) -L/opt/rocm/lib -lamdhip64

clean:
	rm -rf $(OUT)
