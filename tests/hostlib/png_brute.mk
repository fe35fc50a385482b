# Builds tests/_build/png_brute_print: the model of k_png_brute's formulation (tools/models/png_brute_model.h) and the
# driver's launch arithmetic (host/png_brute_launch.h) as a plain C++ program (png_brute_print.cc).
# SANITIZE="-fsanitize=address,undefined" SUFFIX=_san builds it with sanitizers under another name;
# WRONG=3 SUFFIX=_wrong3 builds the model with one rule wrong (1 .. 6, see png_brute_print.cc).
ROOT  := $(abspath ../..)
HOST  := $(ROOT)/zopfli_amd/csrc/host
MODEL := $(ROOT)/tools/models
OUT   := $(ROOT)/tests/_build
SUFFIX ?=
WRONG ?=

all: $(OUT)/png_brute_print$(SUFFIX)
.PHONY: all

$(OUT)/png_brute_print$(SUFFIX): png_brute_print.cc $(MODEL)/png_brute_model.h $(HOST)/png_brute_launch.h
	mkdir -p $(OUT)
	g++ -O2 -std=c++17 -Wall -Wextra $(SANITIZE) $(if $(WRONG),-DPNG_BRUTE_WRONG=$(WRONG)) -I$(MODEL) -I$(HOST) -o $@ png_brute_print.cc
