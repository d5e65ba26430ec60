// Stand-in for the Windows SDK header of this name: the reference's stdafx.h includes it, the files compiled into
// oracle/_ref/libref.so use nothing from it (oracle/Makefile, target _ref/libref.so).
#pragma once
