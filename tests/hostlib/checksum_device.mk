# Builds tests/_build/checksum_device_print: the rules of device/zmx_checksum_device.h and the PNG frame of
# host/device_output_plan.h as a plain C++ program (checksum_device_print.cc), linked with host/checksum.cc.
# SANITIZE="-fsanitize=address,undefined" SUFFIX=_san builds it with sanitizers under another name.
ROOT := $(abspath ../..)
DEV  := $(ROOT)/zopfli_amd/csrc/device
HOST := $(ROOT)/zopfli_amd/csrc/host
OUT  := $(ROOT)/tests/_build
SUFFIX ?=

all: $(OUT)/checksum_device_print$(SUFFIX)
.PHONY: all

$(OUT)/checksum_device_print$(SUFFIX): checksum_device_print.cc $(DEV)/zmx_checksum_device.h $(HOST)/device_output_plan.h \
                                       $(HOST)/png_container.h $(HOST)/checksum.h $(HOST)/checksum.cc
	mkdir -p $(OUT)
	g++ -O1 -std=c++17 -Wall -Wextra $(SANITIZE) -I$(ROOT)/include -I$(DEV) -I$(HOST) -o $@ checksum_device_print.cc $(HOST)/checksum.cc -lpthread
