# Builds tests/_build/png_color_print: the rules of device/zmx_png_color.h and host/png_color_choose.h as a plain C++
# program (png_color_print.cc), and tests/_build/png_prefix_print: host/png_container.h's prefix of a reduced file
# (png_prefix_print.cc, linked with checksum.cc).
# SANITIZE="-fsanitize=address,undefined" SUFFIX=_san builds them with sanitizers under other names.
ROOT := $(abspath ../..)
DEV  := $(ROOT)/zopfli_amd/csrc/device
HOST := $(ROOT)/zopfli_amd/csrc/host
OUT  := $(ROOT)/tests/_build
SUFFIX ?=

all: $(OUT)/png_color_print$(SUFFIX) $(OUT)/png_prefix_print$(SUFFIX)
.PHONY: all

$(OUT)/png_color_print$(SUFFIX): png_color_print.cc $(DEV)/zmx_png_color.h $(HOST)/png_color_choose.h $(ROOT)/include/zopfli_amd.h
	mkdir -p $(OUT)
	g++ -O1 -std=c++17 -Wall -Wextra $(SANITIZE) -I$(DEV) -I$(HOST) -I$(ROOT)/include -o $@ png_color_print.cc

$(OUT)/png_prefix_print$(SUFFIX): png_prefix_print.cc $(HOST)/png_container.h $(HOST)/checksum.h $(HOST)/checksum.cc
	mkdir -p $(OUT)
	g++ -O1 -std=c++17 -Wall -Wextra $(SANITIZE) -I$(HOST) -I$(ROOT)/include -o $@ png_prefix_print.cc $(HOST)/checksum.cc -lpthread
