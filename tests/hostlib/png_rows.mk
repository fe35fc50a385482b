# Builds tests/_build/png_rows_print: the rules of device/zmx_png_rows.h as a plain C++ program (png_rows_print.cc),
# and tests/_build/png_container_print: host/png_container.h around a zlib stream from a file (png_container_print.cc).
# SANITIZE="-fsanitize=address,undefined" SUFFIX=_san builds them with sanitizers under other names.
ROOT := $(abspath ../..)
DEV  := $(ROOT)/zopfli_amd/csrc/device
HOST := $(ROOT)/zopfli_amd/csrc/host
OUT  := $(ROOT)/tests/_build
SUFFIX ?=

all: $(OUT)/png_rows_print$(SUFFIX) $(OUT)/png_container_print$(SUFFIX)
.PHONY: all

$(OUT)/png_rows_print$(SUFFIX): png_rows_print.cc $(DEV)/zmx_png_rows.h
	mkdir -p $(OUT)
	g++ -O1 -std=c++17 -Wall -Wextra $(SANITIZE) -I$(DEV) -o $@ png_rows_print.cc

$(OUT)/png_container_print$(SUFFIX): png_container_print.cc $(HOST)/png_container.h $(HOST)/checksum.h $(HOST)/checksum.cc
	mkdir -p $(OUT)
	g++ -O1 -std=c++17 -Wall -Wextra $(SANITIZE) -I$(HOST) -I$(ROOT)/include -o $@ png_container_print.cc $(HOST)/checksum.cc -lpthread
