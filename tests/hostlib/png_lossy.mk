# Builds tests/_build/png_lossy_print: the rules of device/zmx_png_lossy.h as a plain C++ program (png_lossy_print.cc).
# SANITIZE="-fsanitize=address,undefined" SUFFIX=_san builds it with sanitizers under another name.
ROOT := $(abspath ../..)
DEV  := $(ROOT)/zopfli_amd/csrc/device
OUT  := $(ROOT)/tests/_build
SUFFIX ?=

all: $(OUT)/png_lossy_print$(SUFFIX)
.PHONY: all

$(OUT)/png_lossy_print$(SUFFIX): png_lossy_print.cc $(DEV)/zmx_png_lossy.h $(DEV)/zmx_png_color.h
	mkdir -p $(OUT)
	g++ -O1 -std=c++17 -Wall -Wextra $(SANITIZE) -I$(DEV) -o $@ png_lossy_print.cc
